"""The attention core of csts_amd/csrc/attention.hip (csts_attn_fwd / csts_attn_bwd / csts_attn_probs) restated in float64 torch on the
CPU, the error magnitudes its bars scale with, a Python restatement of the host code's choice of kernels, and the case table.  Not a
test module: tests/test_attention_core_reference_host.py checks it on the CPU, tests/attention_raw.py compares the kernels with it.

The rule is that of include/csts_hip.h, not torch autograd (q, k, v, dO: (B, H, N, hd), already rounded to the storage type):
  z2    = (q . k) scale log2(e), -inf outside the same-frame blocks; frame(x) = x // HW for x < T HW, else x - T HW
  LSE   = log2 sum_k exp2(z2)                                   P = exp2(z2 - LSE)         O = P V
  delta = sum_d dO O_in                                         dP = dO V^T                dS = P_in (dP - delta), P_in = exp2(z2 - LSE_in)
  dQ    = scale dS K                                            dK = scale dS^T Q          dV = P_in^T dO
The backward is handed O_in = O rounded to the storage type and LSE_in = LSE rounded to fp32, both from THIS reference: an error of
the forward kernel can neither hide nor cause a backward failure.  Every output comes with its magnitude A: the same expression with
every operand replaced by its absolute value and no cancellation (|dP| + |delta|, not their difference); A_z = scale log2(e) max_k
sum_d |q| |k| is the magnitude of a row's scores."""
import functools
import math
import os
import zlib

import numpy as np
import torch

LOG2E = math.log2(math.e)
U = 2.0 ** -24
U16 = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}    # unit roundoff of a stored output
STORE = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


# ------------------------------------------------------------------------------------------------------------ the rule
def frame_ids(T, HW):
    n = np.arange(T * HW + T)
    return np.where(n < T * HW, n // HW, n - T * HW)


def live_mask(mask, Nq, Nk):
    """bool (Nq, Nk): True where the query sees the key.  mask: None or (T, HW)."""
    if mask is None:
        return torch.ones(Nq, Nk, dtype=torch.bool)
    f = torch.from_numpy(frame_ids(*mask))
    assert Nq == Nk == f.numel()
    return f[:, None] == f[None, :]


def scale_of(hd):
    return float(np.float32(hd ** -0.5))          # the fp32 value the callers hand the kernels


def forward(q, k, v, scale, mask=None):
    """float64 (B, H, N, hd) -> O, LSE (log2 domain), P, z2, A_O, A_z."""
    live = live_mask(mask, q.shape[2], k.shape[2])
    z2 = (q @ k.transpose(-1, -2)) * (scale * LOG2E)
    z2 = z2.masked_fill(~live, -float("inf"))
    lse = torch.logsumexp(z2 * math.log(2.0), dim=-1) / math.log(2.0)
    P = torch.exp2(z2 - lse[..., None])
    A_z = (scale * LOG2E) * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1)
    return {"O": P @ v, "LSE": lse, "P": P, "z2": z2, "A_O": P @ v.abs(), "A_z": A_z}


def backward(q, k, v, do, o_in, lse_in, scale, z2):
    """float64 operands; o_in / lse_in as the kernel reads them -> delta, dQ, dK, dV and their magnitudes."""
    delta = (do * o_in).sum(-1)
    A_delta = (do.abs() * o_in.abs()).sum(-1)
    P = torch.exp2(z2 - lse_in[..., None])                                  # exp2(-inf) = 0 on masked keys
    dP = do @ v.transpose(-1, -2)
    dS = P * (dP - delta[..., None])
    A_dS = P * (do.abs() @ v.abs().transpose(-1, -2) + A_delta[..., None])
    return {"delta": delta, "A_delta": A_delta, "P_in": P,
            "dQ": scale * (dS @ k), "A_dQ": scale * (A_dS @ k.abs()),
            "dK": scale * (dS.transpose(-1, -2) @ q), "A_dK": scale * (A_dS.transpose(-1, -2) @ q.abs()),
            "dV": P.transpose(-1, -2) @ do, "A_dV": P.transpose(-1, -2) @ do.abs(), "A_dS_max": float(A_dS.max())}


def autograd(q, k, v, do, scale, mask=None):
    """float64 torch autograd of softmax(q k^T scale + mask) v: what the restatement above must be."""
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    live = live_mask(mask, q.shape[2], k.shape[2])
    z = (q @ k.transpose(-1, -2)) * scale
    z = z.masked_fill(~live, -float("inf"))
    o = torch.softmax(z, dim=-1) @ v
    o.backward(do)
    return {"O": o.detach(), "LSE": torch.logsumexp(z.detach(), -1) * LOG2E, "dQ": q.grad, "dK": k.grad, "dV": v.grad}


def frame_of_f32(x, HW):
    """The device form (int)(((float)x + 0.5f) * (1.f / (float)HW)) in numpy float32 arithmetic."""
    inv = np.float32(1.0) / np.float32(HW)
    return ((x.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ the plan
def cdiv(a, b):
    return -(-a // b)


def env_of(environ=None):
    """The four switches as the host code reads them: FWD / DKV / FUSED -> False when set to 0, DQ -> the forced value or -1."""
    e = os.environ if environ is None else environ

    def off(name):
        v = e.get(name)
        return v is not None and _atoi(v) == 0
    dq = e.get("CSTS_ATTN_DQ_FAST")
    return {"fwd_fast": not off("CSTS_ATTN_FWD_FAST"), "dkv_fast": not off("CSTS_ATTN_DKV_FAST"),
            "fused": not off("CSTS_ATTN_FUSED_BWD"), "dq": -1 if dq is None else _atoi(dq)}


def _atoi(s):
    try:
        return int(s.strip())
    except ValueError:
        return 0


def plan(B, H, Nq, Nk, hd, h16, masked, env):
    """attn_launch / fused_bwd_ok / dkv_fast / dq_fast / dkv_plan of attention.hip restated.  h16: the 16-bit type (else fp32).
    -> {"fwd", "path", "dq", "dkv", "nsplit", "q_chunk", "reduce", "ws"}; the kernel names are those of the source."""
    t = "false" if h16 else "true"
    fwd = "attn_fwd_fast_kernel" if env["fwd_fast"] and h16 and hd == 96 and not masked and Nk % 64 == 0 else f"attn_fwd_kernel<{hd},{t}>"
    fused = env["fused"] and h16 and hd == 96 and Nk <= 128 and not masked and Nq >= 1024
    if fused:
        want = max(1, min(256 // (B * H), cdiv(Nq, 256)))
        q_chunk = cdiv(cdiv(Nq, want), 128) * 128
        nsplit = cdiv(Nq, q_chunk)
        dq, dkv, path = None, "attn_bwd_fused_kernel" + ("/direct" if nsplit == 1 else ""), "one-pass"
    else:
        fast = env["dkv_fast"] and h16 and hd == 96 and not masked and Nq % 128 == 0
        qblk = 128 if fast else 64 if hd == 96 else 32
        want = max(1, 256 // (cdiv(Nk, 128) * B * H))
        want = max(1, min(want, cdiv(Nq, 4 * qblk)))
        q_chunk = cdiv(cdiv(Nq, want), qblk) * qblk
        nsplit = cdiv(Nq, q_chunk)
        if env["dq"] == 0 or not h16 or hd != 96 or masked or Nk % 64 != 0:
            dq = f"attn_dq_kernel<{hd},{t}>"
        else:
            dq = "attn_dq_fast_kernel<4>" if env["dq"] == 4 and Nk % 128 == 0 else "attn_dq_fast_kernel<2>"
        if fast:
            dkv = "attn_dkv_kernel<96,false,false>"
        else:
            slow = (not h16) or hd == 96 or masked or Nq % (64 if hd == 96 else 32) != 0
            dkv = f"attn_dkv_kernel<{hd},{t},{'true' if slow else 'false'}>"
        path = "two-kernel"
    ws = 2 * nsplit * B * H * Nk * hd * 4 if nsplit > 1 else 16
    return {"fwd": fwd, "path": path, "dq": dq, "dkv": dkv, "nsplit": nsplit, "q_chunk": q_chunk, "reduce": nsplit > 1, "ws": ws}


# Every instantiation behind the three entry points: 5 forward, 6 dQ, 6 dK/dV, the one-pass kernel (its direct-store branch, taken
# when nsplit == 1, named apart), the reduce and the probabilities.
INSTANTIATIONS = (
    [f"attn_fwd_kernel<{hd},{t}>" for hd in (96, 192) for t in ("true", "false")] + ["attn_fwd_fast_kernel"]
    + [f"attn_dq_kernel<{hd},{t}>" for hd in (96, 192) for t in ("true", "false")] + ["attn_dq_fast_kernel<2>", "attn_dq_fast_kernel<4>"]
    + [f"attn_dkv_kernel<{hd},{t},true>" for hd in (96, 192) for t in ("true", "false")]
    + ["attn_dkv_kernel<192,false,false>", "attn_dkv_kernel<96,false,false>", "attn_bwd_fused_kernel", "attn_bwd_fused_kernel/direct",
       "attn_dkv_reduce_kernel", "attn_probs_kernel"])


# ------------------------------------------------------------------------------------------------------------ the cases
# name -> (B, H, Nq, Nk, head dims, dtypes ("f32", "h16"), mask (T, HW) or None, probs)
CASES = {
    "one_tile": (1, 1, 40, 24, (96, 192), ("f32", "h16"), None, False),
    "ragged_both": (2, 2, 300, 100, (96,), ("f32", "h16"), None, False),
    "whole_fast": (1, 2, 640, 192, (96,), ("f32", "h16"), None, False),
    "whole_single": (1, 1, 256, 256, (96,), ("h16",), None, False),
    "fast_ragged_q": (2, 1, 200, 128, (96,), ("h16",), None, False),
    "hd192_whole": (1, 2, 160, 96, (192,), ("f32", "h16"), None, False),
    "hd192_ragged": (1, 2, 150, 70, (192,), ("f32", "h16"), None, False),
    "fused_ragged": (1, 2, 1100, 100, (96,), ("h16",), None, False),
    "fused_whole": (2, 1, 1024, 128, (96,), ("h16",), None, False),
    "fused_tiny_kv": (1, 1, 1030, 8, (96,), ("h16",), None, False),
    "fused_kv33": (1, 1, 1024, 33, (96,), ("h16",), None, False),
    "fused_single_split": (3, 43, 1024, 8, (96,), ("h16",), None, False),
    "staircase": (1, 1, 128, 512, (96,), ("f32", "h16"), None, False),
    "staircase20": (1, 1, 128, 512, (96,), ("f32", "h16"), None, False),
    "peaked": (1, 2, 200, 100, (96,), ("f32", "h16"), None, False),
    "zero_head": (1, 2, 300, 100, (96,), ("h16",), None, False),
    "dq4_three_tiles": (1, 1, 200, 384, (96,), ("h16",), None, False),          # the dq4 child only
    "mask_3x49": (1, 2, 150, 150, (96,), ("f32", "h16"), (3, 49), True),
    "mask_3x49_hd192": (1, 1, 150, 150, (192,), ("f32", "h16"), (3, 49), True),
    "mask_4x64": (1, 2, 260, 260, (96,), ("f32", "h16"), (4, 64), True),
    "mask_5x1": (1, 1, 10, 10, (96,), ("f32", "h16"), (5, 1), True),
    # found by the mutation check: float(41) * fl(1 / 41) < 1, so the first token of frame 1 is in frame 1 only through the + 0.5f of
    # frame_of (41 is the smallest HW with such a token; HW = 49 and 64 have none below 2^12)
    "mask_2x41": (1, 1, 84, 84, (96,), ("f32", "h16"), (2, 41), True),
    "mask_1x40": (1, 1, 41, 41, (96,), ("f32", "h16"), (1, 40), True),
    "nomask_41": (1, 1, 41, 41, (96,), ("f32", "h16"), None, True),             # the same operands as mask_1x40, unmasked
}
PROBS_CAP = (1, 2, 1024, 600, 96)                                               # probs only, fp32
IN_PROCESS = [n for n in CASES if n != "dq4_three_tiles"]
CHILD_CASES = {
    "generic": ["whole_fast", "whole_single", "fast_ragged_q", "fused_ragged", "fused_tiny_kv", "staircase"],
    "dq4": ["whole_single", "dq4_three_tiles"],
    "fp16": ["one_tile", "ragged_both", "whole_fast", "fast_ragged_q", "hd192_ragged", "fused_ragged", "mask_3x49"],
}
CHILD_ENV = {
    "generic": {"CSTS_ATTN_FWD_FAST": "0", "CSTS_ATTN_DQ_FAST": "0", "CSTS_ATTN_DKV_FAST": "0", "CSTS_ATTN_FUSED_BWD": "0"},
    "dq4": {"CSTS_ATTN_DQ_FAST": "4"},
    "fp16": {},
}
VARIANTS = ("", "_big", "_subnormal")                                           # the fp16 child runs all three
SWITCHES = ("CSTS_ATTN_FWD_FAST", "CSTS_ATTN_DQ_FAST", "CSTS_ATTN_DKV_FAST", "CSTS_ATTN_FUSED_BWD")


def runs(names, half_only=False):
    """(name, hd, dtype key) of every run of the named cases."""
    return [(n, hd, dk) for n in names for hd in CASES[n][4] for dk in CASES[n][5] if not (half_only and dk == "f32")]


def reached(names, env, half_only=False):
    """The set of instantiations the named cases run under `env`."""
    got = set()
    for n, hd, dk in runs(names, half_only):
        B, H, Nq, Nk, _, _, mask, probs = CASES[n]
        p = plan(B, H, Nq, Nk, hd, dk == "h16", mask is not None, env)
        got |= {p["fwd"], p["dkv"]} | ({p["dq"]} if p["dq"] else set()) | ({"attn_dkv_reduce_kernel"} if p["reduce"] else set())
        got |= {"attn_probs_kernel"} if probs else set()
    return got


# ------------------------------------------------------------------------------------------------------------ the operands
STAIR_RISE = {"staircase": 5.0, "staircase20": 20.0}
STAIR_SLOW = 3.0                                      # log2-domain rise per 64-key tile of the slow rows


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _staircase_qk(name, hd, seed):
    """Queries i % 3 == 0 rise by STAIR_RISE per 64-key tile along one direction e, i % 3 == 1 rise by STAIR_SLOW, i % 3 == 2 fall by
    STAIR_RISE.  k = noise + g(tile) e, q = noise orthogonal to e + a e: score = a g scale log2(e) + noise of about one unit."""
    B, H, Nq, Nk = CASES[name][:4]
    rise = STAIR_RISE[name]
    e = _randn((hd,), seed + 50)
    e = e / e.norm()
    qn = 0.5 * _randn((B, H, Nq, hd), seed)
    qn = qn - (qn @ e)[..., None] * e
    a = torch.tensor([4.0, 4.0 * STAIR_SLOW / rise, -4.0])[torch.arange(Nq) % 3]
    g = (rise / (4.0 * hd ** -0.5 * LOG2E)) * (torch.arange(Nk) // 64).float()
    q = qn + a[None, None, :, None] * e
    k = _randn((B, H, Nk, hd), seed + 1) + g[None, None, :, None] * e
    return q, k


def operands(name, hd, store, variant=""):
    """fp32 tensors (B, H, N, hd), rounded to the storage type: q, k, v, dO."""
    B, H, Nq, Nk = CASES[name][:4]
    seed = zlib.crc32(("mask_1x40" if name == "nomask_41" else name).encode()) % 100000 + hd      # nomask_41: the operands of mask_1x40
    if name in STAIR_RISE:
        q, k = _staircase_qk(name, hd, seed)
    else:
        q, k = _randn((B, H, Nq, hd), seed), _randn((B, H, Nk, hd), seed + 1)
    v, do = _randn((B, H, Nk, hd), seed + 2), _randn((B, H, Nq, hd), seed + 3)
    if name == "peaked":
        q = q * 6.0
    if name == "zero_head":
        do[:, 1] = 0.0
    if variant == "_subnormal":                       # every 5th channel of q, k, v in the fp16 subnormal range (|x| < 6.1e-5)
        for t in (q, k, v):
            t[..., ::5] *= 1e-5
    return [t.to(store).float() for t in (q, k, v, do)]


@functools.lru_cache(maxsize=None)
def reference(name, hd, store_key, variant=""):
    """Everything a run of one case is held to, computed once.  store_key: "f32" | "bf16" | "fp16".
    variant "_big" (fp16): the forward runs with V at sigma 4e3, clamped to 3.2e4 (O reaches the top of the fp16 range); the backward
    keeps the ordinary V and scales dO by the largest power of two <= 4096 at which A_dS, A_dQ, A_dK and A_dV stay below 2^15 -- dS
    is rounded to the 16-bit type before the second products, so |dO| |V| cannot both sit at the top of the range."""
    store = STORE[store_key]
    B, H, Nq, Nk, _, _, mask, _ = CASES[name]
    scale = scale_of(hd)
    q, k, v, do = operands(name, hd, store, variant)
    v_fwd = v
    if variant == "_big":
        v_fwd = (v * 4e3).clamp(-3.2e4, 3.2e4).to(store).float()
    q64, k64, v64, do64 = q.double(), k.double(), v.double(), do.double()
    f = forward(q64, k64, v_fwd.double(), scale, mask)
    fb = f if v_fwd is v else forward(q64, k64, v64, scale, mask)
    o_in = fb["O"].to(store).double()
    lse_in = fb["LSE"].float().double()
    b = backward(q64, k64, v64, do64, o_in, lse_in, scale, fb["z2"])
    do_scale = 1.0
    if variant == "_big":
        top = max(b["A_dS_max"], float(b["A_dQ"].max()), float(b["A_dK"].max()), float(b["A_dV"].max()))
        do_scale = min(4096.0, 2.0 ** math.floor(math.log2(2.0 ** 15 / top)))
        do = (do * do_scale).to(store).float()
        b = backward(q64, k64, v64, do.double(), o_in, lse_in, scale, fb["z2"])
    r = {"name": name, "hd": hd, "store": store, "variant": variant, "mask": mask, "scale": scale, "shape": (B, H, Nq, Nk),
         "q": q, "k": k, "v": v, "v_fwd": v_fwd, "do": do, "do_scale": do_scale, "o_in": o_in, "lse_in": lse_in,
         "O": f["O"], "A_O": f["A_O"], "LSE": f["LSE"], "A_z": f["A_z"], "z2": f["z2"], "P_in": b["P_in"]}
    r.update({kk: b[kk] for kk in ("delta", "A_delta", "dQ", "A_dQ", "dK", "A_dK", "dV", "A_dV", "A_dS_max")})
    return r


@functools.lru_cache(maxsize=None)
def probs_cap_reference():
    """PROBS_CAP: q, k fp32, LSE_in, P and A_z (the probabilities alone; 1,228,800 elements)."""
    B, H, Nq, Nk, hd = PROBS_CAP
    q, k = _randn((B, H, Nq, hd), 77), _randn((B, H, Nk, hd), 78)
    f = forward(q.double(), k.double(), torch.zeros(B, H, Nk, hd, dtype=torch.float64), scale_of(hd))
    lse_in = f["LSE"].float().double()
    return {"q": q, "k": k, "lse_in": lse_in, "A_z": f["A_z"], "P_in": torch.exp2(f["z2"] - lse_in[..., None]), "scale": scale_of(hd)}


def rescale_kinds(z2_row_tiles):
    """The forward's lazy running max on the float64 tile maxima of one row (T,) -> (rescales after tile 0, has two tiles in a row
    whose max grew without a rescale, never rescales after tile 0)."""
    m, true_max = -1e30, -float("inf")
    fired, quiet, two_quiet = [], 0, False
    for t, ms in enumerate(z2_row_tiles):
        grow = ms > m + 8.0
        grew = ms > true_max
        true_max = max(true_max, ms)
        if grow:
            m = ms
            quiet = 0
        elif grew and t > 0:
            quiet += 1
            two_quiet = two_quiet or quiet >= 2
        else:
            quiet = 0
        fired.append(grow)
    later = any(fired[1:])
    return later, two_quiet, not later
