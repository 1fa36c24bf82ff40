"""MODEL.ACT_CHECKPOINT without a GPU: the model surface with the key on (which blocks are checkpointed, no "not applied"
warning, the reference's state_dict) and the deferred end-of-backward state under a backward pass that runs inside another
one (csts_amd.ops.nested_backward), driven on CPU tensors with the finishing launches stubbed."""
import copy
import json
import logging
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")


def _build(on, caplog=None):
    from csts_amd.config import load_yaml
    from csts_amd.registry import MODEL_REGISTRY
    cfg = load_yaml(YAML, ["NUM_GPUS", 0, "MODEL.LOSS_FUNC", "kldiv+egonce", "MODEL.ACT_CHECKPOINT", on])
    return MODEL_REGISTRY.get("CSTS")(cfg)


def test_key_on_checkpoints_exactly_the_encoder_blocks(caplog):
    """The 16 video and 4 audio encoder blocks -- the reference's set (custom_multimodal_builder.py:154,178,214) -- and nothing
    else; no warning that the key is not applied; parameters and state_dict as without the key (fairscale's wrapper prefixes
    nothing either)."""
    from csts_amd.model import Block
    with caplog.at_level(logging.INFO, logger="csts_amd"):
        m = _build(True)
    assert not any("not applied" in r.getMessage() for r in caplog.records)
    want = [f"blocks.{i}" for i in range(16)] + [f"blocks_audio.{i}" for i in range(4)]
    assert m.checkpointed_blocks() == want
    for n, b in m.named_modules():
        if isinstance(b, Block):
            assert b.checkpointed == (n in want), n
    for n in ("temporal_fusion", "spatial_fusion", "decode_block1", "decode_block2", "decode_block3", "decode_block4"):
        assert not getattr(m, n).checkpointed
    ref = json.load(open(os.path.join(GOLDEN, "manifest_T8.json")))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref["entries"] and len(ref["entries"]) == 524
    off = _build(False)
    assert off.checkpointed_blocks() == []
    assert list(off.state_dict().keys()) == list(m.state_dict().keys())
    off.load_state_dict(m.state_dict(), strict=True)          # a checkpoint written with the key on loads with it off
    m.load_state_dict(off.state_dict(), strict=True)          # ... and the other way round


def test_key_on_refuses_the_split_stage3_experiment(monkeypatch):
    from csts_amd import model as M
    monkeypatch.setattr(M, "SPLIT_STAGE3", True)
    with pytest.raises(NotImplementedError, match="CSTS_SPLIT_STAGE3"):
        _build(True)
    _build(False)


class _StubLib:
    """Stands in for libcsts_hip.so: records the finishing launches instead of running them."""

    def __init__(self):
        self.calls = []

    def csts_reduce_rows_batched(self, base, n, ncols, stream):
        self.calls.append(("batched", n))
        return 0

    csts_reduce_rows_wide = csts_reduce_rows_batched


class _StubTable:
    def __init__(self, *a, **k):
        self.uploads = 0

    def upload(self, payload):
        self.uploads += 1
        return 4096


@pytest.fixture
def stubbed_ops(monkeypatch):
    from csts_amd import ops
    lib = _StubLib()
    monkeypatch.setattr(ops, "_lib", lambda: lib)
    monkeypatch.setattr(ops, "HostTable", _StubTable)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "DEFER_REDUCTIONS", True)
    monkeypatch.setattr(ops, "_tables", {})
    ops.reset_deferred()
    yield ops, lib
    ops.reset_deferred()
    assert not ops._suspended


def _defer_one(ops, p, value, log):
    """What a first-stage kernel's wrapper does inside a backward pass: queue a reduction and the hand-over of its result."""
    assert ops._can_defer(p)
    g = torch.full_like(p, value)
    ops._defer(torch.zeros(4, p.numel()), g, 4, p.numel())
    ops._assign_later(p, g)
    log.append((torch._C._current_graph_task_id(), len(ops._pass.deferred), len(ops._pass.assign)))


def test_outer_queue_survives_an_inner_pass_and_the_inner_queue_is_finished(stubbed_ops):
    ops, lib = stubbed_ops
    p_outer1, p_outer2, p_inner = (torch.nn.Parameter(torch.zeros(3)) for _ in range(3))
    log, seen = [], {}

    class InnerOp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, g):
            _defer_one(ops, p_inner, 5.0, log)
            return g * 2

    class Deferring(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, p, v):
            ctx.p, ctx.v = p, v
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            _defer_one(ops, ctx.p, ctx.v, log)
            return g, None, None

    class Recompute(torch.autograd.Function):
        """A node that runs a backward pass of its own inside the outer one (what ops.CheckpointFn does)."""

        @staticmethod
        def forward(ctx, x):
            ctx.save_for_backward(x)
            return x * 2

        @staticmethod
        def backward(ctx, g):
            x, = ctx.saved_tensors
            seen["outer_before"] = (len(ops._pass.deferred), len(ops._pass.assign), ops._pass.task)
            with ops.nested_backward(lane=1):
                assert ops._pass.lane == 1 and len(ops._suspended) == 1
                assert not ops._pass.deferred and not ops._pass.assign and ops._pass.task == -1
                with torch.enable_grad():
                    xd = x.detach().requires_grad_(True)
                    y = InnerOp.apply(xd)
                torch.autograd.backward(y, g)
                # the inner pass's own final callback has finished its queue and handed its gradient over
                seen["inner_after"] = (len(ops._pass.deferred), len(ops._pass.assign), ops._pass.task)
                seen["inner_grad"] = None if p_inner.grad is None else p_inner.grad.clone()
                seen["launches_inner"] = list(lib.calls)
            seen["outer_after"] = (len(ops._pass.deferred), len(ops._pass.assign), ops._pass.task)
            seen["outer_grad_mid"] = p_outer1.grad
            return xd.grad

    x = torch.ones(3, requires_grad=True)
    h = Deferring.apply(x, p_outer2, 7.0)       # runs last in backward
    h = Recompute.apply(h)
    out = Deferring.apply(h, p_outer1, 3.0)     # runs first: the outer queue holds its work when the inner pass starts
    out.sum().backward()

    assert seen["outer_before"][0] == 1 and seen["outer_before"][1] == 1 and seen["outer_before"][2] >= 0
    assert seen["inner_after"] == (0, 0, -1)
    assert torch.equal(seen["inner_grad"], torch.full((3,), 5.0))
    assert seen["launches_inner"] == [("batched", 1)]
    assert seen["outer_after"] == seen["outer_before"]          # untouched: same entries, same owner
    assert seen["outer_grad_mid"] is None                       # and not handed over early
    # the outer pass went on queueing under its own id and finished everything at its end, exactly once
    outer_ids = {t for t, _, _ in (log[0], log[2])}
    assert len(outer_ids) == 1 and log[1][0] not in outer_ids
    assert log[2][1:] == (2, 2)
    assert torch.equal(p_outer1.grad, torch.full((3,), 3.0)) and torch.equal(p_outer2.grad, torch.full((3,), 7.0))
    assert torch.equal(p_inner.grad, torch.full((3,), 5.0))
    assert lib.calls == [("batched", 1), ("batched", 2)]
    assert torch.equal(x.grad, torch.full((3,), 2.0))
    assert not ops._pass.deferred and not ops._pass.assign and not ops._suspended and ops._pass.lane is None
    assert {k for kind, k in ops._tables if kind == "reduce"} == {None, ("nested", 1, None)}      # the nested flush read a table of its own lane


def test_inner_pass_that_raises_leaves_the_outer_queue_alone(stubbed_ops):
    ops, lib = stubbed_ops
    p_outer, p_inner = torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(2))
    log = []

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            _defer_one(ops, p_inner, 1.0, log)
            raise RuntimeError("boom")

    class Outer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            _defer_one(ops, p_outer, 9.0, log)
            with ops.nested_backward():
                with torch.enable_grad():
                    xd = g.detach().requires_grad_(True)
                    y = Boom.apply(xd)
                try:
                    torch.autograd.backward(y, g)
                except RuntimeError:
                    pass
            assert len(ops._pass.deferred) == 1 and len(ops._pass.assign) == 1 and ops._pass.assign[0][0] is p_outer
            return g

    x = torch.ones(2, requires_grad=True)
    Outer.apply(x).sum().backward()
    assert torch.equal(p_outer.grad, torch.full((2,), 9.0)) and p_inner.grad is None
    assert lib.calls == [("batched", 1)]


class _FakeStream:
    def __init__(self):
        self.syncs = 0

    def synchronize(self):
        self.syncs += 1


def _fill(ps, stream):
    """Something in every field of a pass (whatever fields it has), `stream` marked as forked."""
    for k, v in vars(ps).items():
        if k == "forked":
            v.append(stream)
        elif isinstance(v, list):
            v.append(("x",))
        elif isinstance(v, dict):
            v["x"] = "x"
        elif k != "lane" and not (k == "task" and v != -1):
            setattr(ps, k, 7)           # the counters, and the task id unless a running pass owns the queues
    assert vars(ps) != vars(type(ps)(ps.lane))


def test_reset_leaves_a_fresh_pass(stubbed_ops):
    ops, lib = stubbed_ops
    st = _FakeStream()
    _fill(ops._pass, st)
    ops.reset_deferred()
    assert st.syncs == 1                                    # launches in flight there read what the reset drops
    assert ops._pass.lane is None and vars(ops._pass) == vars(ops._Pass(None))
    ops.reset_deferred()
    assert st.syncs == 1
    # the same inside a nested pass, with the outer pass untouched
    outer, st_outer, st_inner = ops._pass, _FakeStream(), _FakeStream()
    _fill(outer, st_outer)
    before = {k: copy.copy(v) for k, v in vars(outer).items()}
    with ops.nested_backward(lane=1):
        assert ops._pass is not outer and vars(ops._pass) == vars(ops._Pass(1))
        _fill(ops._pass, st_inner)
        ops.reset_deferred()
        assert st_inner.syncs == 1 and st_outer.syncs == 0
        assert vars(ops._pass) == vars(ops._Pass(1))
        assert ops._suspended == [outer] and vars(outer) == before
    assert ops._pass is outer and vars(outer) == before and not ops._suspended
    assert st_inner.syncs == 1 and st_outer.syncs == 0


# module-level containers of csts_amd.ops that legitimately outlive a backward pass (the comment block above ops._Pass says why);
# everything that belongs to ONE pass is a field of ops._Pass, where reset, suspension and flush reach it without naming it
CROSS_PASS = {"_host_tables", "_suspended", "_w8_total", "_side_streams", "_tables", "_grad_targets", "_grad_targets_used",
              "_wg_plans", "_WG_CLASSES"}


def _containers(ops):
    return {k: v for k, v in vars(ops).items() if isinstance(v, (list, dict, set)) and not k.startswith("__")}


def test_every_pass_field_is_reset_and_framed(stubbed_ops):
    ops, lib = stubbed_ops
    assert set(_containers(ops)) == CROSS_PASS, "per-pass state belongs in ops._Pass, not in a module global"

    class Deferring(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, p, v, log):
            ctx.p, ctx.v, ctx.log = p, v, log
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            _defer_one(ops, ctx.p, ctx.v, ctx.log)
            return g, None, None, None

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            _fill(ops._pass, _FakeStream())     # the pass dies with something in every field
            raise RuntimeError("boom")

    def clean_pass():
        p1, p2, log = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(3)), []
        x = torch.ones(3, requires_grad=True)
        Deferring.apply(Deferring.apply(x, p1, 3.0, log), p2, 7.0, log).sum().backward()
        calls, lib.calls[:] = list(lib.calls), []
        return p1.grad, p2.grad, x.grad, calls, [e[1:] for e in log]

    alone = clean_pass()
    state = {k: copy.copy(v) for k, v in _containers(ops).items()}
    p_dead, log = torch.nn.Parameter(torch.zeros(3)), []
    x = torch.ones(3, requires_grad=True)
    with pytest.raises(RuntimeError, match="boom"):
        Deferring.apply(Boom.apply(x), p_dead, 1.0, log).sum().backward()         # defers, then dies in the next node
    assert len(ops._pass.deferred) == 2 and ops._pass.task == log[0][0] and not lib.calls      # the dead pass's leftovers are still there
    after = clean_pass()
    assert all(torch.equal(a, b) for a, b in zip(alone[:3], after[:3])) and alone[3:] == after[3:]
    assert alone[3] == [("batched", 2)] and p_dead.grad is None
    assert vars(ops._pass) == vars(ops._Pass(None))
    assert _containers(ops) == state
