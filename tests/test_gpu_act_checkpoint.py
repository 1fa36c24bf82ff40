"""MODEL.ACT_CHECKPOINT on the GPU: every video / audio encoder block keeps its input and recomputes its forward in backward
(ops.CheckpointFn).  Checkpointing changes no value in the reference, so the reference fixtures of tests/test_gpu_model.py
are the reference for it, at that file's bars; key on against key off is held to the project's bar for "same arithmetic"
(rel-L2 < 1e-5, test_gradient_accumulation_and_failed_backward).  Every model is built by build_model(cfg) with the key in
the cfg."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2, GOLDEN

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import test_gpu_model as TM                            # noqa: E402  (its bars and fixture checks, unchanged)
from csts_amd import lib as L                          # noqa: E402
from csts_amd.config import load_yaml                  # noqa: E402
from csts_amd.build import build_model                 # noqa: E402
from csts_amd.model import Block                       # noqa: E402
from csts_amd import ops, train as T                   # noqa: E402
from oracle import csts_oracle as O                    # noqa: E402

DEV = torch.device("cuda:0")
YAML = TM.YAML
SAME = 1e-5            # the project's bar for "same arithmetic, other summation grouping"; measured: bit equality, which is what is asserted
# C-ABI launches (lib.check calls) of ONE eager train step at 8 x 256^2, B = 2, bf16 mode, eval-mode model, measured on the commit
# this feature was added to.  With the key off the step must still issue exactly these.
PARENT_LAUNCHES_T8_B2_BF16 = 756


def _model(compute, T_, on, opts=(), yaml=YAML, train=False):
    cfg = load_yaml(yaml, ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", T_, "CSTS_AMD.COMPUTE", compute,
                           "MODEL.ACT_CHECKPOINT", bool(on)] + list(opts))
    m = build_model(cfg)
    m.load_state_dict(O.seeded_params(T_, 256), strict=True)
    assert len(m.checkpointed_blocks()) == (20 if on else 0)
    return (m.train() if train else m.eval()), cfg


def _pass(m, cfg, batch, seed=None, keep_masks=None, zero=True):
    if zero:
        for p in m.parameters():
            p.grad = None
    if seed is not None:
        torch.manual_seed(seed)
    loss, kld, nce, preds = T.compute_loss(cfg, m, batch["video"], batch["audio"], batch["labels_hm"], keep_masks=keep_masks)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), kld.detach(), nce.detach(), preds.detach()


def _grads(m):
    return {n: p.grad.clone() for n, p in m.named_parameters()}


def _same(label, res_on, g_on, res_off, g_off):
    """Losses bit-equal and every one of the 524 gradients bit-equal (backward is bitwise reproducible here, and a checkpointed
    step runs the arithmetic of a plain one); the worst rel-L2 is printed first, against the bar SAME that bit equality implies."""
    assert len(g_on) == len(g_off) == 524
    for a, b in zip(res_on[:3], res_off[:3]):
        assert torch.equal(a, b), (label, float(a), float(b))
    assert torch.equal(res_on[3], res_off[3]), label
    worst, worst_n, unequal = 0.0, "", []
    for n in g_off:
        e = rel_l2(g_on[n], g_off[n])
        if not torch.equal(g_on[n], g_off[n]):
            unequal.append(n)
        if e > worst:
            worst, worst_n = e, n
    print(f"\n[{label}] key on vs off: losses bit-equal, worst gradient rel-L2 {worst:.3e} ({worst_n}), {len(unequal)} of 524 gradients not bit-equal")
    assert worst < SAME, (label, worst_n, worst)
    assert not unequal, (label, unequal[:10])


def test_reference_parity_T8_with_key_on_and_on_equals_off():
    """(3) the parity gate of test_full_model_fp32_vs_reference_golden, same fixture, same bars, same (eval) mode, key on; and
    (4) key on against key off on the same weights and batch."""
    m, cfg = _model("fp32", 8, True)
    g = TM._load("model_T8_B2.npz")
    batch = TM.dev_batch(2, 8, 1000)
    res_on = _pass(m, cfg, batch, seed=3)
    loss, kld, nce, heat = res_on
    assert rel_l2(heat, g["heat"]) < 1e-3
    assert rel_l2(heat, g["heat"]) < 1e-4
    assert (heat.reshape(2, 8, -1).argmax(-1).cpu().numpy() == g["argmax"]).all()
    assert abs(float(kld) - float(g["kld"])) < 1e-4 and abs(float(nce) - float(g["nce"])) < 1e-3
    assert abs(float(loss) - float(g["loss"])) < 1e-4
    named = dict(m.named_parameters())
    for n, ref_norm in zip([str(x) for x in g["grad_names"]], g["grad_norms"]):
        if n == "classifier.bias":
            continue
        gr = named[n].grad
        gnorm = float(gr.double().norm())
        assert abs(gnorm - ref_norm) <= 2e-3 * ref_norm, (n, gnorm, ref_norm)
        assert rel_l2(gr.flatten()[:64], g[n.replace(".", "_") + "_g"]) < 5e-3, n
    total = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters())))
    assert abs(total - float(g["grad_total_norm"])) < 1e-3 * float(g["grad_total_norm"])
    g_on = _grads(m)
    del m, named
    m_off, cfg_off = _model("fp32", 8, False)
    res_off = _pass(m_off, cfg_off, batch, seed=3)
    _same("fp32 T8 B2 eval", res_on, g_on, res_off, _grads(m_off))


def test_reference_parity_T16_train_fixture_with_key_on():
    """(3) model_T16_B2_train.npz at the bars of test_train_T16_fp32_vs_reference_golden."""
    m, cfg = _model("fp32", 16, True)
    g = TM._load("model_T16_B2_train.npz")
    loss, kld, nce, preds = TM._train_pass(m, cfg, TM.dev_batch(2, 16, 1004))
    assert rel_l2(preds.flatten()[:4096], g["heat_head"]) < 1e-4
    TM._check_train_fixture(m, g, loss, kld, nce, preds, loss_tol=1e-4, norm_tol=2e-3, slice_tol=5e-3, total_tol=1e-3,
                            argmax_min=1.0, label="fp32 T16 B2, ACT_CHECKPOINT")


def test_injected_drop_path_masks_are_what_the_recompute_uses():
    """(3) keep_masks= (the reference's recorded draws, model_T8_B2_droppath.npz) through a grad-enabled forward + backward: the
    forward equals the fixture and key on equals key off."""
    g = TM._load("model_T8_B2_droppath.npz")
    rnd = torch.from_numpy(g["rand"])
    active = [s for s in O.derive_geometry()["video"] if s.drop_path > 0]
    km = {}
    for i, s in enumerate(active):
        keep = 1.0 - s.drop_path
        km[s.prefix] = (torch.floor(keep + rnd[2 * i]), torch.floor(keep + rnd[2 * i + 1]))
    assert any(float(v[0].min()) == 0.0 or float(v[1].min()) == 0.0 for v in km.values())      # some branch is really dropped
    batch = TM.dev_batch(2, 8, 1000)
    out = {}
    for on in (True, False):
        m, cfg = _model("fp32", 8, on)
        logits = m([batch["video"]], batch["audio"], keep_masks=km)
        assert rel_l2(logits, g["logits"]) < 1e-4
        res = _pass(m, cfg, batch, keep_masks=km)
        out[on] = (res, _grads(m))
        del m
    _same("fp32 T8 B2, injected drop-path masks", out[True][0], out[True][1], out[False][0], out[False][1])


@pytest.mark.parametrize("compute,grouped", [("fp32", False), ("bf16", False), ("bf16", True)])
def test_dropout_and_drop_path_masks_are_replayed(compute, grouped, monkeypatch):
    """(5) train mode, MVIT.DROPOUT_RATE 0.1 and the YAML's DROPPATH_RATE 0.2: equal losses and gradients prove that the recompute
    sees every mask again.  grouped: the weight gradients queued and finished per block by the nested pass (what a captured
    step does), against ONE grouped tail with the key off."""
    if grouped:
        monkeypatch.setattr(ops, "GROUP_WGRADS", "always")
    batch = T.synthetic_batch(2, 8, 256, 41, DEV)
    out = {}
    for on in (True, False):
        m, cfg = _model(compute, 8, on, ["MVIT.DROPOUT_RATE", 0.1], train=True)
        assert cfg.MVIT.DROPPATH_RATE == 0.2 and m.blocks[-1].drop_prob > 0
        res = _pass(m, cfg, batch, seed=11)
        out[on] = (res, _grads(m))
        del m
    ops.reset_deferred()
    _same(f"{compute} T8 B2 train, dropout 0.1, drop-path 0.2, grouped={grouped}", out[True][0], out[True][1], out[False][0], out[False][1])
    eval_loss = _pass(*_model(compute, 8, False), batch)[0]
    assert not torch.equal(eval_loss, out[False][0][0])        # the masks were really on


def _graph_nodes(root):
    seen, stack, nodes = set(), [root], []
    while stack:
        n = stack.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        nodes.append(n)
        stack.extend(fn for fn, _ in n.next_functions)
    return nodes


def test_it_really_checkpoints_and_accumulates():
    """(6) after a forward with the key on, the tape holds ONE node per encoder block and that node keeps the block input only; no
    LayerNorm / Linear / MLP / attention node of an encoder block exists.  A second backward without zeroing accumulates to the
    key-off model's p.grad += g."""
    batch = T.synthetic_batch(2, 8, 256, 5, DEV)
    m, cfg = _model("fp32", 8, True)
    loss, *_ = T.compute_loss(cfg, m, batch["video"], batch["audio"], batch["labels_hm"])
    nodes = _graph_nodes(loss.grad_fn)
    names = [type(n).__name__ for n in nodes]
    ck = [n for n in nodes if type(n).__name__ == "CheckpointFnBackward"]
    assert len(ck) == 20
    blocks = {id(b): n for n, b in m.named_modules() if isinstance(b, Block)}
    assert sorted(blocks[id(n.block)] for n in ck) == sorted(m.checkpointed_blocks())
    for n in ck:
        saved = n.saved_tensors
        assert len(saved) == 1 and saved[0].dim() == 3 and saved[0].shape[-1] == n.block.dim
    # what is left of the per-block node types belongs to the 6 fusion / decoder blocks
    assert names.count("MlpFnBackward") == 6 and names.count("AttnInnerFnBackward") == 6
    assert names.count("LayerNormFnBackward") == 12
    m_off, cfg_off = _model("fp32", 8, False)
    loss_off, *_ = T.compute_loss(cfg_off, m_off, batch["video"], batch["audio"], batch["labels_hm"])
    names_off = [type(n).__name__ for n in _graph_nodes(loss_off.grad_fn)]
    assert names_off.count("MlpFnBackward") == 26 and "CheckpointFnBackward" not in names_off
    loss.backward()
    loss_off.backward()
    res_on = _pass(m, cfg, batch, zero=False)             # second step, accumulated
    res_off = _pass(m_off, cfg_off, batch, zero=False)
    _same("fp32 T8 B2, two accumulated steps", res_on, _grads(m), res_off, _grads(m_off))
    one = _pass(m_off, cfg_off, batch)
    assert rel_l2(m.blocks[5].mlp.fc1.weight.grad, 2 * m_off.blocks[5].mlp.fc1.weight.grad) < SAME and float(one[0]) == float(res_off[0])


def test_peak_memory_T32():
    """(7) one eager forward + backward at 32 x 256^2, B = 1, bf16: peak allocated bytes with the key on against off (off is what
    the code did before the key was honoured).  Floor from shapes alone: the saving is at least the MLP pre-activation h and
    activation g of the sixteen video blocks.  Measured on MI355X: see R_MEASURED."""
    aria = os.path.join(os.path.dirname(YAML), "..", "Aria", "CSTS_Aria_Gaze_Forecast.yaml")
    b = TM.dev_batch(1, 32, 1003)
    peak, losses = {}, {}
    floor = 0
    for on in (False, True):
        m, cfg = _model("bf16", 32, on, yaml=aria)
        if on:
            thw = list(m.patch_dims)
            for blk in m.blocks:
                if blk.has_pool_q:
                    thw = [(t - 1) // s + 1 for t, s in zip(thw, blk.stride_q)]
                floor += 2 * (thw[0] * thw[1] * thw[2]) * blk.mlp.fc1.out_features * 2          # h and g, 2 bytes each, B = 1
        _pass(m, cfg, b)                                  # allocator warm, lazily built tables in place
        for p in m.parameters():
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        losses[on] = _pass(m, cfg, b)[0]
        peak[on] = torch.cuda.max_memory_allocated()
        print(f"\n[bf16 T32 B1, ACT_CHECKPOINT {on}] peak allocated {peak[on] / 2**30:.3f} GiB (model and batch resident: {base / 2**30:.3f} GiB)")
        del m
    r = peak[True] / peak[False]
    print(f"[bf16 T32 B1] peak on / off = {r:.4f}; floor from shapes (h + g of 16 video blocks) {floor / 2**30:.3f} GiB, saved {(peak[False] - peak[True]) / 2**30:.3f} GiB")
    assert torch.equal(losses[True], losses[False])
    assert peak[False] - peak[True] >= floor
    assert r <= (1.0 + R_MEASURED) / 2.0, (r, R_MEASURED)


R_MEASURED = 0.6641     # peak on / off of the test above on MI355X (5.023 -> 3.336 GiB); the bar is (1 + r) / 2: losing half of the saving fails


def test_graphed_train_step_matches_eager_with_key_on():
    """(8) bars of test_graphed_train_step_matches_eager, three steps."""
    m, cfg = _model("bf16", 8, True)
    m2 = copy.deepcopy(m)
    assert len(m2.checkpointed_blocks()) == 20
    batch = T.synthetic_batch(2, 8, 256, 99, DEV)
    opt_e = T.construct_optimizer(m, cfg)
    opt_g = T.construct_optimizer(m2, cfg, capturable=True)
    state0 = copy.deepcopy(m2.state_dict())
    g = T.GraphedTrainStep(cfg, m2, opt_g, batch, warmup=1)
    m2.load_state_dict(state0)
    opt_g.reset_state() if hasattr(opt_g, "reset_state") else opt_g.state.clear()
    le = [float(T.train_step(cfg, m, batch, opt_e, lr=1e-4)[0]) for _ in range(3)]
    lg = [float(g.run(batch, lr=1e-4)[0]) for _ in range(3)]
    print(f"\n[graphed step, ACT_CHECKPOINT] eager losses {le}, replayed {lg}")
    assert abs(le[0] - lg[0]) < 1e-4 and abs(le[1] - lg[1]) < 5e-3 and abs(le[2] - lg[2]) < 5e-3, (le, lg)
    assert rel_l2(m2.blocks[5].mlp.fc1.weight, m.blocks[5].mlp.fc1.weight) < 1e-3
    ops.reset_deferred()


@pytest.mark.parametrize("trunk_cut", [3, 0])
def test_segmented_train_step_matches_eager_with_key_on(trunk_cut):
    """(8) bars of test_segmented_train_step_matches_eager, three steps."""
    m, cfg = _model("bf16", 8, True)
    cfg.CSTS_AMD.TRUNK_CUT = trunk_cut
    m2 = copy.deepcopy(m)
    batch = T.synthetic_batch(2, 8, 256, 99, DEV)
    opt_e = T.construct_optimizer(m, cfg)
    opt_g = T.construct_optimizer(m2, cfg, capturable=True)
    state0 = copy.deepcopy(m2.state_dict())
    g = T.SegmentedTrainStep(cfg, m2, opt_g, batch, warmup=1)
    assert g.trunk_cut == trunk_cut and ("bwd_trunk_early" in g.graphs) == bool(trunk_cut)
    m2.load_state_dict(state0)
    opt_g.reset_state()
    le = [float(T.train_step(cfg, m, batch, opt_e, lr=1e-4)[0]) for _ in range(3)]
    lg = [float(g.run(batch, lr=1e-4)[0]) for _ in range(3)]
    print(f"\n[segmented step, ACT_CHECKPOINT, trunk_cut={trunk_cut}] eager losses {le}, graph-chain losses {lg}")
    assert abs(le[0] - lg[0]) < 1e-4 and abs(le[1] - lg[1]) < 5e-3 and abs(le[2] - lg[2]) < 5e-3, (le, lg)
    for name in ("blocks.5.mlp.fc1.weight", "blocks_audio.2.attn.pool_k.weight", "vision_pool.weight", "decode_block3.norm1.weight",
                 "pos_embed_spatial", "classifier.weight", "blocks.1.mlp.fc1.weight", "blocks.2.attn.qkv.weight",
                 "patch_embed.proj.weight", "blocks.3.norm1.weight"):
        w_e, w_g = dict(m.named_parameters())[name], dict(m2.named_parameters())[name]
        assert rel_l2(w_g, w_e) < 1e-3, name
    ops.reset_deferred()


def _count_launches(m, cfg, batch, monkeypatch):
    T.train_step(cfg, m, batch)                           # lazily built tables, allocator
    calls = [0]
    real = L.check

    def counting(rc, what=""):
        calls[0] += 1
        return real(rc, what)

    monkeypatch.setattr(L, "check", counting)
    try:
        T.train_step(cfg, m, batch)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(L, "check", real)
    return calls[0]


def test_key_off_costs_nothing(monkeypatch):
    """(9) the C-ABI launches of one eager step with the key off are the count of the commit before the feature; with the key on the
    step adds the twenty recomputed block forwards (every one a C-ABI launch: no torch-op fallback) and twenty small finishing
    launches."""
    batch = T.synthetic_batch(2, 8, 256, 77, DEV)
    m_off, cfg_off = _model("bf16", 8, False)
    n_off = _count_launches(m_off, cfg_off, batch, monkeypatch)
    m_on, cfg_on = _model("bf16", 8, True)
    n_on = _count_launches(m_on, cfg_on, batch, monkeypatch)
    print(f"\n[bf16 T8 B2 eager step] C-ABI launches: key off {n_off}, key on {n_on}")
    assert n_off == PARENT_LAUNCHES_T8_B2_BF16
    assert n_on > n_off
