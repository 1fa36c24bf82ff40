"""Raw C-ABI item tables for the grouped weight-gradient kernels (csts_wgrad_grouped8 / _limited, csts_wgrad_grouped5,
csts_wgrad_grouped) and their fp64 reference.  Shared by tests/test_gpu_wgrad.py (bf16 library) and tests/fp16_wgrad_worker.py
(fp16 library, child process); not a test module itself.

Every output of a table (one weight-gradient tile set over one token range, or one interleaved stage set) gets its own fp32
buffer, laid out as GUARD floats, M rows of ldc > N floats, GUARD floats, all filled with a NaN sentinel bit pattern before the
launch.  After it, every element of the M x N region must be finite and every other element still the sentinel: the kernel wrote
its whole tile and nothing beside it.  The reference is dW = dY64^T X64 and db = colsum(dY64) over the output's token rows, from
the operands AFTER rounding to the 16-bit type the kernel reads (an fp32 dY is rounded as the staging rounds it), so that the
only remaining error is fp32 accumulation: |err| <= c 2^-24 (|dY|^T |X|) element-wise, c ~ the sequential additions."""
import torch

from csts_amd import lib as L

U = 2.0 ** -24
GUARD = 64                       # floats before and after every output (keeps 16-byte alignment)
SENT = 0x7FC0DEAD                # a quiet NaN no kernel produces
C_DW, C_DB = 8.0, 1.5            # element-wise bars in units of 2^-24 x the absolute product / sum (measured worst: 2.4 / 0.39)


def _sentinel(n, dev):
    return torch.full((n,), SENT, dtype=torch.int32, device=dev).view(torch.float32)


class Out:
    """One fp32 target [M][ldc] between guard bands (dW, or db when rows == 1 and the target is a vector)."""

    def __init__(self, M, N, ldc, dev):
        self.M, self.N, self.ldc = M, N, ldc
        self.buf = _sentinel(GUARD + M * ldc + GUARD, dev)
        self.mask = torch.zeros(self.buf.numel(), dtype=torch.bool, device=dev)
        self.mask[GUARD:GUARD + M * ldc].view(M, ldc)[:, :N] = True

    def ptr(self):
        return self.buf.data_ptr() + GUARD * 4

    def reset(self):
        self.buf.view(torch.int32).fill_(SENT)

    def tile(self):
        return self.buf[GUARD:GUARD + self.M * self.ldc].view(self.M, self.ldc)[:, :self.N]

    def guards_ok(self):
        return bool((self.buf.view(torch.int32)[~self.mask] == SENT).all())

    def untouched(self):
        return bool((self.buf.view(torch.int32) == SENT).all())


class Problem:
    """dW[M, N] = dY[:, M]^T X[:, N] over `tokens` rows, dY / X read in place from wider row-major buffers (column offsets
    aoff / boff, 16-byte aligned), one output per token range in `ranges`: (kbeg, kend, step) -- step > 1: the 16-token
    stages kbeg, kbeg + 16 step, ... < kend (csts_wgrad_grouped5's interleaved items, item field M = step)."""

    def __init__(self, M, N, tokens, ranges, colsum, dev, seed, a_dt, h_dt, big=False, subnormal=False, lpad=(64, 32),
                 offs=(8, 16)):
        self.M, self.N, self.tokens, self.ranges, self.colsum = M, N, tokens, ranges, colsum
        g = torch.Generator().manual_seed(seed)
        aoff, boff = offs
        self.lda, self.ldb = M + lpad[0], N + lpad[1]
        ya = torch.randn(tokens, self.lda, generator=g)
        xb = torch.randn(tokens, self.ldb, generator=g)
        if big:             # |x| up to ~3e4 (IEEE half tops out at 65504): the products and sums stay far inside fp32
            ya = (ya * 1e4).clamp(-3.2e4, 3.2e4)
            xb = (xb * 1e4).clamp(-3.2e4, 3.2e4)
        if subnormal:       # every 5th feature of dY and every 7th of X in the fp16 subnormal range (|x| < 6.1e-5)
            ya[:, ::5] *= 1e-5
            xb[:, ::7] *= 1e-5
        self.ybuf = ya.to(dev).to(a_dt)
        self.xbuf = xb.to(dev).to(h_dt)
        self.dY = self.ybuf[:, aoff:aoff + M]
        self.X = self.xbuf[:, boff:boff + N]
        assert (self.dY.data_ptr() % 16 == 0 and self.X.data_ptr() % 16 == 0 and self.lda * self.ybuf.element_size() % 16 == 0
                and self.ldb * 2 % 16 == 0)
        ldc = (N + 8 + 3) // 4 * 4
        self.outs = [Out(M, N, ldc, dev) for _ in ranges]
        self.css = [Out(1, M, M, dev) if colsum else None for _ in ranges]
        self.stray = Out(1, M, M, dev)           # the colsum target of every n0 != 0 item: must stay untouched
        dY64 = self.dY.to(h_dt).double()         # the 16-bit operand the kernel multiplies (fp32 dY: rounded as staged)
        X64 = self.X.double()
        self.ref = []
        for kb, ke, step in ranges:
            rows = self.rows(kb, ke, step)
            A, B = dY64[rows], X64[rows]
            self.ref.append((A.t() @ B, A.abs().t() @ B.abs(), A.sum(0), A.abs().sum(0), int(rows.numel())))

    def rows(self, kb, ke, step):
        if step <= 1:
            return torch.arange(kb, ke, device=self.dY.device)
        st = torch.arange(kb, ke, 16 * step, device=self.dY.device)
        return (st[:, None] + torch.arange(16, device=self.dY.device)[None, :]).flatten()

    def items(self, tm, tn, w5=False):
        """One WgradItem per (output, tile): m0 over range(0, M, tm), n0 over range(0, N, tn)."""
        its = []
        for (kb, ke, step), out, cs in zip(self.ranges, self.outs, self.css):
            for m0 in range(0, self.M, tm):
                for n0 in range(0, self.N, tn):
                    it = L.WgradItem()
                    it.A, it.B, it.C = self.dY.data_ptr(), self.X.data_ptr(), out.ptr()
                    it.colsum = (cs.ptr() if n0 == 0 else self.stray.ptr()) if cs is not None else None
                    it.lda, it.ldb, it.ldc = self.lda, self.ldb, out.ldc
                    it.kbeg, it.kend = kb, ke
                    it.M, it.N, it.m0, it.n0 = (step if w5 else self.M), self.N, m0, n0
                    its.append(it)
        return its

    def reset(self):
        for o in self.outs + [c for c in self.css if c is not None] + [self.stray]:
            o.reset()

    def check(self):
        """Per output: rel-L2 of dW (and db) against fp64, the worst |err| / (2^-24 |dY|^T |X|) and its bound c, guard bands."""
        res = []
        for out, cs, (ref, absref, dbref, absdb, ntok) in zip(self.outs, self.css, self.ref):
            t = out.tile().double()
            err = (t - ref).abs()
            r = {"tokens": ntok, "finite": bool(torch.isfinite(t).all()), "guards": out.guards_ok(),
                 "rel": float((t - ref).norm() / ref.norm()),
                 "ratio": float(torch.where(absref > 0, err / (U * absref), err * float("inf")).nan_to_num(0.0).max()),
                 "c": min(ntok / 16 + 17, C_DW), "stray": self.stray.untouched()}
            if cs is not None:
                d = cs.tile().double().flatten()
                e = (d - dbref).abs()
                r.update(db_finite=bool(torch.isfinite(d).all()), db_guards=cs.guards_ok(), db_rel=float((d - dbref).norm() / dbref.norm()),
                         db_ratio=float(torch.where(absdb > 0, e / (U * absdb), e * float("inf")).nan_to_num(0.0).max()), db_c=min(ntok + 16, C_DB))
            res.append(r)
        return res

    def snapshot(self):
        return [o.buf.clone() for o in self.outs] + [c.buf.clone() for c in self.css if c is not None]


def upload(items, dev, pad_every=0):
    """Device copy of the item list; pad_every > 0 inserts an A == NULL padding slot after every pad_every items; the
    table is padded to a multiple of 8 entries.  Returns (device tensor, entry count)."""
    seq = []
    for i, it in enumerate(items):
        seq.append(it)
        if pad_every and i % pad_every == pad_every - 1:
            seq.append(L.WgradItem())
    while len(seq) % 8:
        seq.append(L.WgradItem())
    arr = (L.WgradItem * len(seq))(*seq)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev), len(seq)


def worst(results, key):
    return max(r[key] for rs in results for r in rs if key in r)


def violations(results, rel_bar, db_rel_bar):
    """Human-readable list of every output that misses a bar (empty: all pass)."""
    bad = []
    for pi, rs in enumerate(results):
        for oi, r in enumerate(rs):
            if not (r["finite"] and r["guards"] and r["stray"] and r["rel"] <= rel_bar and r["ratio"] <= r["c"]):
                bad.append((pi, oi, {k: r[k] for k in ("finite", "guards", "stray", "rel", "ratio", "c")}))
            if "db_rel" in r and not (r["db_finite"] and r["db_guards"] and r["db_rel"] <= db_rel_bar and r["db_ratio"] <= r["db_c"]):
                bad.append((pi, oi, {k: r[k] for k in ("db_finite", "db_guards", "db_rel", "db_ratio", "db_c")}))
    return bad


def _stream():
    return torch.cuda.current_stream().cuda_stream


def launch(kind, table, n, **kw):
    lib = L.load()
    if kind == "w8":
        rc = lib.csts_wgrad_grouped8(table.data_ptr(), n, _stream())
    elif kind == "w8l":
        rc = lib.csts_wgrad_grouped8_limited(table.data_ptr(), n, kw["max_wgs"], _stream())
    elif kind == "w5":
        rc = lib.csts_wgrad_grouped5(table.data_ptr(), n, _stream())
    else:
        rc = lib.csts_wgrad_grouped(table.data_ptr(), n, kw["a_f32"], kw["rows"], _stream())
    L.check(rc, kind)


# --------------------------------------------------------------------------------------------- the problem sets
def w8_problems(dev, h_dt, **kw):
    """192 x 384 class: one- and multi-tile layers, token ranges of 64 / 128 / 192 / 8192, ranges that start inside the
    tokens (kbeg != 0) and end before them, colsum given and NULL."""
    return [
        Problem(192, 384, 64, [(0, 64, 1)], True, dev, 11, h_dt, h_dt, **kw),
        Problem(1152, 384, 320, [(0, 128, 1), (128, 320, 1)], True, dev, 12, h_dt, h_dt, **kw),
        Problem(384, 1536, 8192, [(0, 8192, 1)], False, dev, 13, h_dt, h_dt, **kw),
        Problem(2304, 768, 512, [(64, 256, 1), (256, 448, 1)], True, dev, 14, h_dt, h_dt, **kw),
    ]


def w8_items(probs):
    """Colsum items (n0 == 0 tiles with a bias target) first, as one run -- a workgroup of the limited launch then walks
    several of them in a row -- then the rest."""
    its = [(p, it) for p in probs for it in p.items(192, 384)]
    first = [it for p, it in its if p.colsum and it.n0 == 0]
    rest = [it for p, it in its if not (p.colsum and it.n0 == 0)]
    return first + rest


def w5_problems(dev, h_dt, **kw):
    """96 x 96 per-wave class: contiguous ranges (M field 0) incl. one of 2064 tokens, an interleaved pair (step 2: stages
    0, 2, 4 ... and 1, 3, 5 ... of 4112 tokens, each item its own output), a layer of 192 x 96 with colsum."""
    return [
        Problem(96, 288, 4112, [(0, 2048, 1), (2048, 4112, 1)], True, dev, 21, h_dt, h_dt, **kw),
        Problem(192, 96, 4112, [(0, 4112, 2), (16, 4112, 2)], True, dev, 22, h_dt, h_dt, **kw),
        Problem(288, 192, 160, [(32, 160, 1)], False, dev, 23, h_dt, h_dt, **kw),
    ]


def wg_problems(dev, a_dt, h_dt, **kw):
    """128-wide classes: ragged shapes (M, N not multiples of the tile), a ragged last range, colsum given and NULL."""
    return [
        Problem(200, 136, 300, [(0, 128, 1), (128, 300, 1)], True, dev, 31, a_dt, h_dt, **kw),
        Problem(256, 384, 1024, [(0, 1024, 1)], True, dev, 32, a_dt, h_dt, **kw),
        Problem(72, 264, 520, [(64, 520, 1)], False, dev, 33, a_dt, h_dt, **kw),
    ]
