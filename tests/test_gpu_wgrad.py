"""Grouped weight gradients against fp64: dW = dY64^T X64 and db = colsum(dY64) from the operands after rounding to the 16-bit type
the kernel reads (tests/wgrad_raw.py), so that the only error left is fp32 accumulation and the bars can be tight.

Covered: csts_wgrad_grouped8 through hand-built item tables (one- and multi-tile layers, token ranges of 64 ... 8192, kbeg != 0,
colsum given and NULL, padding slots, operands read in place from wider buffers, outputs between sentinel guard bands);
csts_wgrad_grouped8_limited on the same tables at every grid size that matters (bit-identical to the full launch);
csts_wgrad_grouped5 and csts_wgrad_grouped (both dY types) on raw tables; the host path (ops.queue_wgrad -> ops.flush_wgrads ->
the deferred slab reductions) on a problem list that reaches every tile class, checked through ops.WG_STATS; the in-line split-K
path; the early 192 x 384 flush on the side stream with a wrong guess of the problem count in both directions, and a pass that
dies with that launch in flight; a captured
flush replayed with new operands; and the fp16 library (tests/fp16_wgrad_worker.py, child process).

Bars: rel-L2 per dW / db at about 4x the worst value measured on MI355X (constants below).  Element-wise,
|err| <= c 2^-24 (|dY|^T |X|) for dW and |err| <= c 2^-24 colsum(|dY|) for db, with c the smaller of the worst-case bound of the
summation order (tokens / 16 + 17 for dW: one rounding per 16-token MFMA step plus the slab sum; tokens + 16 for db) and
R.C_DW = 8 / R.C_DB = 1.5 -- measured worst 2.4 (dW, fp16 grouped8) and 0.39 (db, fp16 grouped8).

Mutation check (scratch builds of wgrad8.hip, arithmetic-only changes: one k-tile fewer, three of four colsum slices folded, the
A fragment's chunk rotation keyed on row & 1): every one fails 12 tests here; the earlier suite misses the colsum mutant entirely
and catches the short k-loop only through test_graphed_train_step_matches_eager."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected everywhere, run only on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import lib as L          # noqa: E402
from csts_amd import ops               # noqa: E402
import wgrad_raw as R                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
H = torch.bfloat16

# rel-L2 bars per dW / db, about 4x the worst measured on MI355X (in the comments); the element-wise bars are R.C_DW / R.C_DB
REL_RAW = 2e-6          # raw tables, dW: 5.7e-7 (grouped8), 2.7e-7 (grouped5), 1.8e-7 (grouped)
REL_RAW_DB = 2e-7       # raw tables, db: 6.5e-9 (grouped8), 4.9e-8 (grouped5), 2.5e-8 (grouped)
REL_HOST = 2e-6         # host path, in-line path, early flush, captured flush, dW: 5.7e-7 (host), 1.5e-7 (in-line)
REL_HOST_DB = 3e-7      # ... db: 5.8e-8 (host), 7.6e-8 (in-line)
REL_FP16 = 2e-6         # fp16 library, dW: 5.8e-7
REL_FP16_DB = 4e-7      # fp16 library, db: 9.8e-8


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    """The tile-class switches at their defaults whatever the environment says (the assertions name the classes)."""
    for k, v in (("WGRAD8", True), ("WGRAD5", True), ("WGRAD5_STRIDED", True), ("W8_EARLY_WGS", 0),
                 ("WGRAD8_CHUNK", 8192), ("WGRAD5_CHUNK", 4096), ("WGRAD_CHUNK", 8192), ("WGRAD5_MIN", 96),
                 ("DEFER_REDUCTIONS", True)):
        monkeypatch.setattr(ops, k, v)
    ops.reset_deferred()
    yield
    ops.reset_deferred()


def _report(name, results):
    print(f"\n[{name}] worst rel {R.worst(results, 'rel'):.3e}  db_rel {R.worst(results, 'db_rel'):.3e}  "
          f"ratio {R.worst(results, 'ratio'):.2f}  db_ratio {R.worst(results, 'db_ratio'):.2f}")


# ------------------------------------------------------------------------------------------------ raw tables, 192 x 384
@pytest.fixture(scope="module")
def w8_table():
    probs = R.w8_problems(DEV, H)
    table, n = R.upload(R.w8_items(probs), DEV, pad_every=7)
    R.launch("w8", table, n)
    torch.cuda.synchronize()
    res = [p.check() for p in probs]
    return probs, table, n, res, [p.snapshot() for p in probs]


def test_wgrad8_raw_table_vs_fp64(w8_table):
    """csts_wgrad_grouped8 on a hand-built table: every dW / db within the fp64 bars, every tile element written (finite where
    the buffer was NaN), nothing outside the tiles touched (guard bands and row gaps keep the sentinel), db written only by
    n0 == 0 items (the n0 != 0 items of a colsum layer point at a second target, which must stay untouched)."""
    probs, table, n, res, _ = w8_table
    _report("wgrad8 raw", res)
    assert len(res) == 4 and sum(len(r) for r in res) == 6
    assert not R.violations(res, REL_RAW, REL_RAW_DB), R.violations(res, REL_RAW, REL_RAW_DB)


@pytest.mark.parametrize("which", ["0", "1", "8", "9", "64", "n-1", "n", "2n"])
def test_wgrad8_limited_bitwise(w8_table, which):
    """csts_wgrad_grouped8_limited on the same table and max_wgs in {0, 1, 8, 9, 64, n - 1, n, 2n}: bit-identical to the full
    launch (an item's arithmetic does not depend on the grid) and so within the same fp64 bars.  With 8 workgroups every one walks
    ~10 items, several colsum items in a row (the table starts with them): the bias reduction reuses the ring's LDS between items."""
    probs, table, n, _, snap = w8_table
    mw = {"n-1": n - 1, "n": n, "2n": 2 * n}.get(which) or int(which)
    for p in probs:
        p.reset()
    R.launch("w8l", table, n, max_wgs=mw)
    torch.cuda.synchronize()
    for p, s in zip(probs, snap):
        got = p.snapshot()
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, s)), (which, p.M, p.N)
    res = [p.check() for p in probs]
    assert not R.violations(res, REL_RAW, REL_RAW_DB)


# ------------------------------------------------------------------------------------------------ raw tables, 96 and 128 classes
def test_wgrad5_raw_table_vs_fp64():
    """csts_wgrad_grouped5 (96 x 96 tiles, one item per wave): contiguous and interleaved (M = stage step) items, token counts that
    are multiples of 16 only, colsum, padding slots."""
    probs = R.w5_problems(DEV, H)
    table, n = R.upload([it for p in probs for it in p.items(96, 96, w5=True)], DEV, pad_every=5)
    R.launch("w5", table, n)
    torch.cuda.synchronize()
    res = [p.check() for p in probs]
    _report("wgrad5 raw", res)
    assert not R.violations(res, REL_RAW, REL_RAW_DB), R.violations(res, REL_RAW, REL_RAW_DB)


@pytest.mark.parametrize("a_f32,rows", [(0, 256), (0, 128), (0, 64), (1, 128), (1, 64)])
def test_wgrad_grouped_raw_table_vs_fp64(a_f32, rows):
    """csts_wgrad_grouped, every tile height and both dY types (fp32 dY is rounded to the 16-bit type while staging: the
    reference rounds it the same way), ragged shapes and token ranges."""
    probs = R.wg_problems(DEV, torch.float32 if a_f32 else H, H)
    table, n = R.upload([it for p in probs for it in p.items(rows, 128)], DEV, pad_every=3)
    R.launch("wg", table, n, a_f32=a_f32, rows=rows)
    torch.cuda.synchronize()
    res = [p.check() for p in probs]
    _report(f"wgrad grouped a_f32={a_f32} rows={rows}", res)
    assert not R.violations(res, REL_RAW, REL_RAW_DB), R.violations(res, REL_RAW, REL_RAW_DB)


# ------------------------------------------------------------------------------------------------ host path
def _ref64(dY, X):
    d = dY.to(L.half_dtype()).double()
    x = X.double()
    return d.t() @ x, d.abs().t() @ x.abs(), d.sum(0), d.abs().sum(0)


def _check_grad(W, b, dY, X, bar, db_bar, what):
    """rel-L2 and the element-wise bound of one layer's gradients against fp64 (c: all tokens in one sequential sum of 16-token
    MFMA steps plus the chunk slabs -- a valid bound for every class)."""
    ref, absref, dbref, absdb = _ref64(dY, X)
    T = dY.shape[0]
    g = W.grad.double()
    assert bool(torch.isfinite(g).all()), what
    rel = float((g - ref).norm() / ref.norm())
    ratio = float(((g - ref).abs() / (R.U * absref).clamp_min(1e-300)).max())
    assert rel <= bar and ratio <= min(T / 16 + T / 4096 + 17, R.C_DW), (what, rel, ratio)
    out = {"rel": rel, "ratio": ratio}
    if b is not None:
        d = b.grad.double()
        db_rel = float((d - dbref).norm() / dbref.norm())
        db_ratio = float(((d - dbref).abs() / (R.U * absdb).clamp_min(1e-300)).max())
        assert db_rel <= db_bar and db_ratio <= min(T + 16, R.C_DB), (what, db_rel, db_ratio)
        out.update(db_rel=db_rel, db_ratio=db_ratio)
    return out


class _Queue(torch.autograd.Function):
    """Backward queues the given weight-gradient problems (ops.queue_wgrad) exactly as LinearFn does; the end-of-backward callback
    (ops.flush_deferred -> ops.flush_wgrads) then launches them and hands the gradients to the parameters."""

    @staticmethod
    def forward(ctx, z, probs, *params):
        ctx.probs = probs
        return z.clone()

    @staticmethod
    def backward(ctx, g):
        for dY, X, W, b in ctx.probs:
            assert ops.queue_wgrad(dY, X, X.shape[0], dY.shape[1], X.shape[1], W, b)
        return (g, None) + (None,) * (2 * len(ctx.probs))


def _host_problems():
    """(name, tokens, N out, K in, dY dtype, bias) reaching every tile class, ragged last chunks (several chunks: partial slabs
    summed by csts_reduce_rows_wide for dW and csts_reduce_rows_batched for db), and a 192 x 384-shaped layer whose token count is
    not a multiple of 64 (it must go to the 96 class)."""
    return [
        ("w8_1chunk", 4096, 192, 384, H, True, "192"),
        ("w8_ragged", 8192 + 64, 384, 768, H, True, "192"),
        ("w8_nobias", 8192, 576, 384, H, False, "192"),
        ("w5_ragged", 4096 + 48, 96, 288, H, True, "96"),
        ("w8_shape_tok16", 4112, 192, 384, H, True, "96"),
        ("c256_ragged", 8192 + 104, 256, 200, H, True, "256"),
        ("c128", 1000, 200, 136, H, True, "128"),
        ("c128_thin", 8192 + 8, 72, 64, H, False, "128"),
        ("f32_ragged", 8192 + 200, 136, 264, torch.float32, True, "128f"),
        ("f32_w8shape", 512, 192, 384, torch.float32, True, "128f"),
    ]


def _make_layers(spec, seed):
    g = torch.Generator().manual_seed(seed)
    layers = []
    for i, (name, T, N, K, dt, bias, cls) in enumerate(spec):
        dY = torch.randn(T, N, generator=g).to(DEV).to(dt)
        X = torch.randn(T, K, generator=g).to(DEV).to(H)
        W = torch.zeros(N, K, device=DEV, requires_grad=True)
        b = torch.zeros(N, device=DEV, requires_grad=True) if bias else None
        layers.append((name, dY, X, W, b, cls))
    return layers


_ENTRY = {"192": "csts_wgrad_grouped8", "96": "csts_wgrad_grouped5", "256": "csts_wgrad_grouped", "128": "csts_wgrad_grouped",
          "128f": "csts_wgrad_grouped"}


def test_host_flush_every_class_vs_fp64(monkeypatch):
    """ops.queue_wgrad -> ops.flush_deferred / ops.flush_wgrads with GROUP_WGRADS = "always": ops.WG_STATS must list exactly one
    launch per tile class -- 192 (csts_wgrad_grouped8), 96 strided (csts_wgrad_grouped5), 256, 128 and fp32-dY 128
    (csts_wgrad_grouped) -- with the FLOP of the problems this test put in that class, and every dW / db equals fp64."""
    monkeypatch.setattr(ops, "GROUP_WGRADS", "always")
    monkeypatch.setattr(ops, "WG_STATS", [])
    spec = _host_problems()
    layers = _make_layers(spec, 5)
    z = torch.zeros(1, device=DEV, requires_grad=True)
    params = [t for _, _, _, W, b, _ in layers for t in (W, b)]
    _Queue.apply(z, [(dY, X, W, b) for _, dY, X, W, b, _ in layers], *params).sum().backward()
    torch.cuda.synchronize()
    want = {}
    for name, T, N, K, dt, bias, cls in spec:
        want[cls] = want.get(cls, 0.0) + 2.0 * T * N * K
    got = sorted((e[0], e[2]) for e in ops.WG_STATS)
    assert got == sorted((_ENTRY[c], f) for c, f in want.items()), got
    assert set(want) == {"192", "96", "256", "128", "128f"}
    worst = {}
    for name, dY, X, W, b, cls in layers:
        r = _check_grad(W, b, dY, X, REL_HOST, REL_HOST_DB, name)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"\n[host flush] {worst}")


def test_inline_split_k_path_vs_fp64(monkeypatch):
    """The in-line weight gradients (GROUP_WGRADS = "never": split-K GEMMs + colsum, through ops.linear backward) on the same
    shapes, same fp64 bar."""
    monkeypatch.setattr(ops, "GROUP_WGRADS", "never")
    worst = {}
    for name, dY, X, W, b, cls in _make_layers(_host_problems(), 6):
        y = ops.linear(X, W, b, out_dt=L.BF16 if dY.dtype == H else L.F32, compute=L.BF16)
        y.backward(dY)
        torch.cuda.synchronize()
        r = _check_grad(W, b, dY, X, REL_HOST, REL_HOST_DB, name)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"\n[inline] {worst}")


def _linear_pass(layers):
    for _, _, _, W, b, _ in layers:
        W.grad = None
        if b is not None:
            b.grad = None
    ys = [ops.linear(X, W, b, out_dt=L.BF16, compute=L.BF16) for _, dY, X, W, b, _ in layers]
    torch.autograd.backward(ys, [dY for _, dY, _, _, _, _ in layers])
    torch.cuda.synchronize()
    return [(W.grad.clone(), b.grad.clone() if b is not None else None) for _, _, _, W, b, _ in layers]


def test_early_wgrad8_flush_wrong_guess_both_ways(monkeypatch):
    """W8_EARLY_WGS > 0 through ops.linear backward (the real side stream and final join): a pass counts the 192 x 384 problems
    (4), the next has FEWER (3: the guess is never reached, everything goes to the final launch), the next MORE (5: the early
    launch fires at the third, two go to the final one), then the same count again (5: early launch at the last).  Every pass
    equals fp64 and, bitwise, the default path."""
    monkeypatch.setattr(ops, "GROUP_WGRADS", "always")
    spec = [(f"w8_{i}", 2048 * (i % 3 + 1), 192 * (i % 2 + 1), 384 * (2 - i % 2), H, i % 2 == 0, "192") for i in range(5)]
    spec.append(("w5", 4096, 96, 288, H, True, "96"))
    layers = _make_layers(spec, 9)
    w8 = [lay for lay in layers if lay[5] == "192"]
    other = [lay for lay in layers if lay[5] != "192"]
    sets = [w8[:4] + other, w8[:3] + other, w8 + other, w8 + other]
    monkeypatch.setattr(ops, "W8_EARLY_WGS", 0)
    default = [_linear_pass(s) for s in sets[:3]]
    monkeypatch.setattr(ops, "W8_EARLY_WGS", 64)
    ops._w8_total[0] = 0
    early = []
    for s in sets:
        early.append(_linear_pass(s))
        assert ops._w8_total[0] == sum(1 for lay in s if lay[5] == "192")
    for s, a, b_ in zip(sets, early, default + [default[2]]):
        for lay, (gw, gb), (dw, db) in zip(s, a, b_):
            assert torch.equal(gw, dw) and (gb is None or torch.equal(gb, db)), lay[0]
            name, dY, X, W, b, cls = lay
            W.grad = gw
            if b is not None:
                b.grad = gb
            _check_grad(W, b, dY, X, REL_HOST, REL_HOST_DB, name)


class _Boom(torch.autograd.Function):
    """A node whose backward raises once the early launch of the pass is on the side stream."""

    @staticmethod
    def forward(ctx, z):
        return z.clone()

    @staticmethod
    def backward(ctx, g):
        assert ops._pass.forked and not ops._pass.wgq and ops._pass.keep      # early launch enqueued, its operands held
        raise RuntimeError("boom")


def test_dead_pass_with_early_flush_in_flight(monkeypatch):
    """W8_EARLY_WGS > 0, four 192 x 384-class layers (tokens 64 k, one and several tiles): a pass counts them, a clean pass launches
    them early; then a pass whose LAST backward node raises a Python exception with that early launch in flight on the side stream
    (its final callback, and so the join, never run); then a clean pass again.  The pass after the dead one must wait for the side
    stream before it drops the dead pass's operands and must start from empty queues: its dW / db are bit-identical to the clean
    pass before, and equal fp64."""
    monkeypatch.setattr(ops, "GROUP_WGRADS", "always")
    monkeypatch.setattr(ops, "W8_EARLY_WGS", 64)
    spec = [("w8_a", 256, 192, 384, H, True, "192"), ("w8_b", 320, 384, 384, H, False, "192"),
            ("w8_c", 448, 192, 768, H, True, "192"), ("w8_d", 576, 384, 768, H, True, "192")]
    layers = _make_layers(spec, 21)
    ops._w8_total[0] = 0
    _linear_pass(layers)                                      # counts
    assert ops._w8_total[0] == 4
    clean = _linear_pass(layers)                              # early launch at the fourth problem
    z = torch.zeros(1, device=DEV, requires_grad=True)
    r = _Boom.apply(z)                                        # made first: the lowest sequence number, so backward runs it last
    ys = [ops.linear(X, W, b, out_dt=L.BF16, compute=L.BF16) for _, dY, X, W, b, _ in layers]
    with pytest.raises(RuntimeError, match="boom"):
        torch.autograd.backward(ys + [r], [dY for _, dY, _, _, _, _ in layers] + [torch.ones_like(r)])
    assert ops._pass.forked and ops._pass.assign              # the dead pass's leftovers, a launch in flight among them
    after = _linear_pass(layers)
    assert not ops._pass.forked and not ops._pass.assign and ops._w8_total[0] == 4
    for lay, (gw, gb), (cw, cb) in zip(layers, after, clean):
        name, dY, X, W, b, cls = lay
        assert torch.equal(gw, cw) and (gb is None or torch.equal(gb, cb)), name
        _check_grad(W, b, dY, X, REL_HOST, REL_HOST_DB, name)


def test_captured_flush_replays_with_new_operands(monkeypatch):
    """One problem set (192 with two chunks, 96, 128, fp32-dY) flushed inside torch.cuda.graph capture, on ONE stream (no early
    flush, no stencil gradients, nothing forked), then replayed twice with new operand contents copied in place: each replay matches
    its own fp64 reference (the captured table upload and slab reductions are what the train step replays)."""
    monkeypatch.setattr(ops, "GROUP_WGRADS", "always")
    spec = [("w8", 8192 + 128, 192, 384, H, True, "192"), ("w5", 4096 + 32, 96, 192, H, True, "96"),
            ("c128", 600, 200, 136, H, True, "128"), ("f32", 700, 136, 264, torch.float32, True, "128f")]
    layers = _make_layers(spec, 12)
    params = [t for _, _, _, W, b, _ in layers for t in (W, b)]
    z = torch.zeros(1, device=DEV, requires_grad=True)
    probs = [(dY, X, W, b) for _, dY, X, W, b, _ in layers]

    def step():
        _Queue.apply(z, probs, *params).sum().backward()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            for p in params:
                p.grad = None
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(77)
    for rep in range(2):
        for _, dY, X, W, b, _ in layers:
            dY.copy_(torch.randn(dY.shape, generator=g).to(DEV).to(dY.dtype))
            X.copy_(torch.randn(X.shape, generator=g).to(DEV).to(X.dtype))
        graph.replay()
        torch.cuda.synchronize()
        for name, dY, X, W, b, _ in layers:
            _check_grad(W, b, dY, X, REL_HOST, REL_HOST_DB, f"{name} replay {rep}")
    del graph


# ------------------------------------------------------------------------------------------------ fp16 library
@pytest.fixture(scope="module")
def fp16_wgrad_results(tmp_path_factory):
    out = tmp_path_factory.mktemp("fp16wg") / "wgrad.json"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CSTS_HALF")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fp16_wgrad_worker.py"), str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    return json.load(open(out))


@pytest.mark.parametrize("case", ["w8", "w8_big", "w8_subnormal", "w5", "w5_big", "w5_subnormal", "wg_h16", "wg_h16_big",
                                  "wg_f32", "wg_f32_subnormal"])
def test_fp16_library_raw_tables_vs_fp64(fp16_wgrad_results, case):
    """libcsts_hip_f16.so: csts_wgrad_grouped8, csts_wgrad_grouped5 and csts_wgrad_grouped (both a_f32 forms) on raw tables with
    IEEE-half operands -- ordinary values, values near the top of the fp16 range (|x| ~ 3e4) and features in the fp16 subnormal
    range -- within the same fp64 bars."""
    r = fp16_wgrad_results
    assert r["half_kind"] == 1
    res = r[case]
    _report(f"fp16 {case}", res)
    assert not R.violations(res, REL_FP16, REL_FP16_DB), R.violations(res, REL_FP16, REL_FP16_DB)
