"""What a kernel READS: every entry with its inputs flush against NaN, on NaN scratch.

The workspace contract file checks what a kernel writes.  Almost every kernel here works in
16-row tiles, loads the last tile whole and masks afterwards - often by multiplication (a zero
row of the gradient against whatever ``x`` holds, a softmax weight of 0) - and many sum partial
tables out of a grow-only scratch buffer.  A load that really leaves its buffer, a partial nobody
wrote or an output element no kernel wrote reads, in every other test, finite numbers of another
tensor or of the previous call, and the result moves by nothing.  Here every entry runs twice on
the same seeded data:

  plain   ordinary tensors, the normal grow-only ``_workspace``;
  flush   every tensor argument copied into an exact slice of a guarded arena
          (``GuardedArena.place``: 256-byte aligned start, last byte against the guard), scratch
          from the same arena with its contents poisoned (``fill_byte=0xFF``), and the call inside
          ``poisoned_fresh_tensors`` (``torch.empty`` and its kin hand out NaN).

Floating inputs get 0xFF guards: NaN in f32 / f64 / bf16 / f16, and NaN x 0 is NaN, so a stray
read "masked" by a zero multiplier reaches the result.  Integer inputs (indices, pointers,
labels, batch vectors) get 0x00 guards: a stray index reads 0, in range for every table here, so
a leak shows as a changed result and not as a bad address.  Asserted for every entry: the guards
are intact, every floating output is finite, the outputs are bit-identical to the plain run.
Where the library sums with float atomics (the attention backward in target order and the
packed / per-node / generic routes) there are no bits to compare: those run in
``attention_backward_order("source")`` for the bit comparison, and in their own order for
finiteness plus the entry's own oracle and bar (tests/test_attention_gpu.py).  The problem
builders and the bars are those of the entries' own test files; no reference is written here.

Limits, so that nobody over-reads a green run:
  * a stray read whose value is truly discarded (a select after the load) is NOT detected - that
    needs page protection and a fault, which these tests must never provoke;
  * integer inputs get the weaker probe (index 0), fresh integer tensors are not poisoned;
  * every stray read lands inside the same live allocation (1 MiB guards against rows of at
    most 1 KiB x 16): a NaN is arithmetic, the tests cannot make a kernel touch memory it would
    not touch anyway;
  * flush are the ARGUMENTS of the call under test.  What a wrapper allocates between its kernels
    (a gradient handed from one layer to the next, the attention's tile records) is an ordinary
    allocation, NaN-filled when fresh and floating, with allocator slack behind it.  Hence the
    second kind of test here: where a kernel's operands are such intermediates it is called once
    more with them as arguments - the fused MLP's backward on flush saved activations
    (``ops._fmlp_backward``), every fused layer, the pool-fused top layer and the segment max
    with the folded norm at the C ABI, segment and attention kernels on flush CSR views;
  * the atomic attention routes meet their f64 oracle in the default precision only (bf16 and
    f32-exact: finite outputs and the forward's bits).

Left out, and why:
  * the plain fused MLP with bf16 STORAGE: it exists only in front of the max-pool
    (test_fused_mlp_maxpool in the bf16 mode at 65 555 rows, and the per-layer cases, run it);
  * batches with a graph that has no rows: rows = 1 runs with one graph, three graphs run from
    17 rows up, every graph with rows;
  * the attention backward's tile records, source list and target view as flush operands:
    ``EdgeCSR`` builds them itself, as integer allocations, from the row pointers, permutation and
    sorted targets that the flush-csr cases place flush; the kernels that make them run on flush
    inputs;
  * the backward of ``gather_rows`` / ``edge_affinity_features`` on a flush CSR view: both sort
    the index inside their autograd node; the same segment-sum kernel reads flush views in
    test_segment_reduce_and_backward;
  * ``spt_fused_linear_bwd_pooled_runs_gn_f32`` / ``spt_fused_linear_bwd_runs_gn_f32`` (the variants
    with the table kernel in their post launch) as C-ABI cases of their own: they run inside
    ``ops._fmlp_backward`` on flush activations; the per-layer cases call the plain entries.
"""
import ctypes
import zlib

import pytest
import torch

from guarded import GuardedArena, exact_workspaces, poisoned_fresh_tensors

pytestmark = pytest.mark.gpu

ROWS = [1, 17, 16 * 131 + 5]


# ---- plumbing -------------------------------------------------------------------------------------
def L():
    from superpoint_transformer_amd import _lib
    return _lib


def seeded(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def flat(x):
    if x is None:
        return []
    if torch.is_tensor(x):
        return [x]
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [t for y in x for t in flat(y)]
    return [torch.as_tensor(x)]


def same_bits(a, b, what):
    fa, fb = flat(a), flat(b)
    assert len(fa) == len(fb), what
    for i, (s, t) in enumerate(zip(fa, fb)):
        assert s.shape == t.shape and s.dtype == t.dtype, (what, i, s.shape, t.shape, s.dtype, t.dtype)
        s8 = s.detach().contiguous().reshape(-1).view(torch.uint8)
        t8 = t.detach().contiguous().reshape(-1).view(torch.uint8)
        if not torch.equal(s8, t8):
            bad = (s.detach().reshape(-1) != t.detach().reshape(-1)) | (s.detach().reshape(-1) != s.detach().reshape(-1))
            raise AssertionError(f"{what}: output {i} {tuple(s.shape)} differs between the plain and the flush run: "
                                 f"{int(bad.sum())} elements, first at flat index {int(bad.nonzero()[0])}")


def all_finite(res, what):
    for i, t in enumerate(flat(res)):
        if t.is_floating_point():
            bad = ~torch.isfinite(t.detach())
            assert not bool(bad.any()), (f"{what}: output {i} {tuple(t.shape)} has {int(bad.sum())} non-finite "
                                         f"elements, first at flat index {int(bad.reshape(-1).nonzero()[0])}")


def plain_put(dev):
    def put(t):
        return None if t is None else t.detach().to(dev).clone()
    return put


def flush_put(dev, arena):
    def put(t, label=None):
        if t is None:
            return None
        t = t.detach().to(dev)
        return arena.place(t, guard_byte=0xFF if t.is_floating_point() else 0x00, label=label)
    return put


def both(dev, fn, what, bits_of=None):
    """``fn(put)`` twice: ``put`` moves a CPU tensor to the device - as an ordinary tensor, then
    flush into a poisoned arena with poisoned scratch and poisoned fresh tensors.  Guards intact,
    floating outputs finite, same bits (``bits_of`` picks the part of the result that has bits to
    compare; False: none).  Returns (plain, flush)."""
    with torch.cuda.device(dev):
        plain = fn(plain_put(dev))
        arena = GuardedArena(dev, guard_byte=0xFF, fill_byte=0xFF)
        with poisoned_fresh_tensors(dev):
            with exact_workspaces(arena):                    # checks every guard on the way out
                from superpoint_transformer_amd import ops
                assert bool(torch.isnan(torch.empty(3, device=dev)).all())          # the probe is armed
                assert bool(torch.isnan(ops._workspace(64, dev).view(torch.float32)).all())
                got = fn(flush_put(dev, arena))
                torch.cuda.synchronize(dev)
    arena.check()
    all_finite(plain, what + " (plain run)")
    all_finite(got, what + " (flush run)")
    if bits_of is not False:
        pick = bits_of or (lambda r: r)
        same_bits(pick(plain), pick(got), what)
    return plain, got


def ok(st, name):
    L().check(st, name)


def P(t):
    return L().ptr(t)


def sp(dev):
    return L().stream_ptr(dev)


def seg_index(g, n, num_seg):
    """An unsorted segment index with empty segments where there is room: the last one, and
    (from 4 segments up) segment 1."""
    idx = torch.randint(0, max(1, num_seg - 1), (n,), generator=g)
    if num_seg > 3:
        idx[idx == 1] = 0
    return idx


def segment_view(put, idx, num_seg, views):
    """The segment index as the wrappers take it: the int64 vector (they sort it into a CSR view of
    their own), or - ``views`` - a ``SegmentCSR`` whose index, ``perm`` and ``rowptr`` are flush too."""
    from superpoint_transformer_amd import csr
    i = put(idx)
    if not views:
        return i
    c = csr.build_csr(i, num_seg)
    return csr.SegmentCSR(i, put(c.perm), put(c.rowptr), c.n, c.num_seg)


def edge_view(put, ei, n, views):
    """The edge list as ``ops.edge_attention`` takes it: [2, E], or - ``views`` - an ``EdgeCSR`` whose
    row pointers, permutation and sorted targets are flush."""
    from superpoint_transformer_amd import csr
    e = put(ei)
    if not views:
        return e
    ec = csr.edge_csr_of(e, n)
    return csr.EdgeCSR(put(ec.erowptr), put(ec.eperm), put(ec.tgt_sorted), n, ec.e)


def test_the_probe_is_armed_on_the_device(dev):
    """What tests/test_guarded_cpu.py shows on the CPU, on the device's memory: one row past a
    flush tensor reads NaN behind a 0xFF guard, a number nothing notices behind 0xA5, zero behind
    an index tensor; poisoned scratch and fresh tensors read NaN."""
    x = torch.randn(7, 5, generator=seeded("armed")) + 3
    zero = torch.tensor([1.0] * 7 + [0.0]).view(8, 1).to(dev)
    nan = GuardedArena(dev, guard_byte=0xFF, fill_byte=0xFF)
    old = GuardedArena(dev)
    past = lambda t: torch.as_strided(t, (8, 5), (5, 1))
    assert bool(torch.isnan((past(nan.place(x.to(dev))) * zero)[7]).all())
    masked = past(old.place(x.to(dev))) * zero
    assert torch.equal(masked[:7].cpu(), x) and bool((masked[7] == 0).all())
    i = nan.place(torch.arange(1, 6).to(dev), guard_byte=0x00)
    assert torch.as_strided(i, (6,), (1,)).tolist() == [1, 2, 3, 4, 5, 0]
    assert bool(torch.isnan(nan.take(64).view(torch.float32)).all())
    with poisoned_fresh_tensors(dev):
        assert bool(torch.isnan(torch.empty(5, device=dev)).all()) and bool(torch.isnan(torch.empty_like(zero)).all())
        assert torch.empty(5, device=dev, dtype=torch.int64).dtype == torch.int64
    assert not hasattr(torch.empty, "__wrapped__")                    # the patch is gone
    nan.check()
    old.check()


def sorted_batch(rows, B):
    return (torch.arange(rows) * B // rows) if B > 1 else None


# ---- segment reductions, gathers ------------------------------------------------------------------------
SEG_CASES = [(1, 1, 4), (17, 5, 7), (2101, 300, 64), (2101, 40, 128), (2101, 700, 3),
             (65_536 + 19, 900, 128)]          # the last: the row-streaming max (c = 128, n >= 65 536)


@pytest.mark.parametrize("views", [False, True], ids=["index", "flush-csr"])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
@pytest.mark.parametrize("n,num_seg,c", SEG_CASES)
def test_segment_reduce_and_backward(n, num_seg, c, reduce, views, dev):
    from superpoint_transformer_amd import ops
    g = seeded("segred", n, num_seg, c)
    x, idx = torch.randn(n, c, generator=g), seg_index(g, n, num_seg)
    gout = torch.randn(num_seg, c, generator=g)
    want_arg = reduce in ("max", "min")

    def fn(put):
        xd, i, go = put(x).requires_grad_(), segment_view(put, idx, num_seg, views), put(gout)
        res = ops.segment_reduce(xd, i, num_seg, reduce, return_arg=want_arg)
        out = res[0] if want_arg else res
        (gx,) = torch.autograd.grad(out, xd, go)
        return res, gx

    both(dev, fn, f"segment_reduce {reduce} {n}x{c}/{num_seg} views={views}")


@pytest.mark.parametrize("n,num_src,c", [(1, 1, 4), (17, 40, 7), (2101, 37, 64), (2101, 5000, 128)])
def test_gather_rows_and_backward(n, num_src, c, dev):
    from superpoint_transformer_amd import ops
    g = seeded("gather", n, num_src, c)
    x = torch.randn(num_src, c, generator=g)
    idx = torch.randint(0, num_src, (n,), generator=g)
    gout = torch.randn(n, c, generator=g)

    def fn(put):
        xd, i, go = put(x).requires_grad_(), put(idx), put(gout)
        out = ops.gather_rows(xd, i)
        (gx,) = torch.autograd.grad(out, xd, go)
        return out, gx

    both(dev, fn, f"gather_rows {n} of {num_src}x{c}")


@pytest.mark.parametrize("n,num_seg,c", [(1, 1, 1), (17, 5, 1), (2101, 300, 1), (2101, 40, 3)])
def test_segment_sum_i64(n, num_seg, c, dev):
    from superpoint_transformer_amd import ops
    g = seeded("sumi64", n, num_seg, c)
    x = torch.randint(-(1 << 40), 1 << 40, (n, c), generator=g)
    idx = seg_index(g, n, num_seg)
    plain, _ = both(dev, lambda put: ops.segment_sum_i64(put(x), put(idx), num_seg), f"segment_sum_i64 {n}x{c}")
    assert torch.equal(plain.cpu(), torch.zeros(num_seg, c, dtype=torch.long).index_add_(0, idx, x))


@pytest.mark.parametrize("n,num_seg", [(1, 1), (17, 5), (2101, 300), (4097, 257), (4097, 65_537)])
def test_csr_build_adopt_and_pos_seg(n, num_seg, dev):
    """``csr_build`` on a flush index, ``pos_seg`` of its view, and ``adopt_csr`` of the same
    partition given as flush (pointers, points)."""
    from superpoint_transformer_amd import csr
    from oracle import spt_oracle as O
    g = seeded("csr", n, num_seg)
    idx = seg_index(g, n, num_seg)
    idx[0] = num_seg - 1 if n > 1 else 0
    rperm, rrow = O.csr_view(idx, num_seg)

    def fn(put):
        i = put(idx)
        c = csr.build_csr(i, num_seg)
        pos = c.pos_seg()
        j = put(idx)                                          # a second tensor: nothing memoised on it
        a = csr.adopt_csr(j, num_seg, put(rrow.long()), put(rperm.long()))
        assert a is not None, "the partition's own CSR was not adopted"
        return c.perm, c.rowptr, pos, a.perm, a.rowptr

    plain, _ = both(dev, fn, f"csr_build / adopt_csr n={n} num_seg={num_seg}")
    perm, rowptr, pos, aperm, arow = (t.cpu() for t in plain)
    assert torch.equal(perm, rperm) and torch.equal(rowptr, rrow) and torch.equal(aperm, rperm) and torch.equal(arow, rrow)
    assert torch.equal(pos.long(), idx[rperm.long()])


# ---- norms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("views", [False, True], ids=["index", "flush-csr"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n,nseg", [(1, 1), (17, 5), (2101, 37), (6147, 3), (2101, None)])
def test_unit_sphere_norm_and_assemble(n, nseg, weighted, views, dev):
    """(6147, 3): segments of 2049 rows, the sliced route; ``nseg=None``: ``idx=None``."""
    from superpoint_transformer_amd import ops
    g = seeded("usn", n, nseg)
    pos = (torch.randn(n, 3, generator=g) * 5 + 20).float()
    # (every segment has rows: the diameter of an empty one is not a number to compare)
    idx = None if nseg is None else (torch.arange(n) % nseg)[torch.randperm(n, generator=g)]
    w = torch.randint(1, 300, (n,), generator=g) if weighted else None
    x = torch.randn(n, 8, generator=g)
    gout = torch.randn(n, 12, generator=g)

    def fn(put):
        view = (lambda: None) if idx is None else (lambda: segment_view(put, idx, nseg, views))
        o, d = ops.unit_sphere_norm(put(pos), view(), put(w), nseg)
        xd = put(x).requires_grad_()
        cat, d2 = ops.unit_sphere_assemble(xd, put(pos), view(), put(w), nseg)
        (gx,) = torch.autograd.grad(cat, xd, put(gout))
        return o, d, cat, d2, gx

    both(dev, fn, f"unit_sphere_norm / assemble n={n} nseg={nseg} weighted={weighted}")


@pytest.mark.parametrize("r,d,B,slope", [(1, 32, 1, 1.0), (17, 64, 3, 0.01), (2101, 128, 3, 0.01), (2101, 32, 1, 0.01),
                                         (2101, 128, 40, 0.01), (60_000, 128, 40, 0.01)])
def test_graph_norm_forward_backward(r, d, B, slope, dev):
    """B = 40 at d = 128: two graph windows of the LDS table; 60 000 rows: at the 128-block floor
    (the case of tests/test_workspace_contract_gpu.py::test_graph_norm)."""
    from superpoint_transformer_amd import ops
    g = seeded("gn", r, d, B)
    x = (torch.randn(r, d, generator=g) * 2 + 3).float()
    batch = sorted_batch(r, B)
    w, b = torch.randn(d, generator=g), torch.randn(d, generator=g)
    a = 1 + 0.3 * torch.randn(d, generator=g)
    gy = torch.randn(r, d, generator=g)

    def fn(put):
        xd = put(x).requires_grad_()
        ps = [put(t).requires_grad_() for t in (w, b, a)]
        y = ops.graph_norm(xd, put(batch), *ps, eps=1e-5, num_graphs=B, act_slope=slope)
        return (y.detach(), *torch.autograd.grad(y, [xd] + ps, put(gy)))

    both(dev, fn, f"graph_norm {r}x{d} B={B}")


# ---- the tall-skinny Linears ---------------------------------------------------------------------------------------
SKINNY = [(64, 192), (64, 64), (128, 128)]
SKINNY_MODES = [0, 1, 3]                                  # f32 pipe, split bf16 (the default), bf16


def skinny_inputs(rows, K, N):
    g = seeded("skinny", rows, K, N)
    return (torch.randn(rows, N, generator=g), torch.randn(rows, K, generator=g),
            torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g))


def pre_tables(rows, K, B):
    g = seeded("pre", rows, K, B)
    return (torch.randn(B, K, generator=g), torch.rand(B, K, generator=g) + 0.5, torch.randn(K, generator=g),
            sorted_batch(rows, B))


@pytest.mark.parametrize("mode", SKINNY_MODES)
@pytest.mark.parametrize("K,N", SKINNY + [(64, 13)])
@pytest.mark.parametrize("rows", ROWS)
def test_skinny_linear_forward_and_input_gradient(rows, K, N, mode, dev):
    """y = x W^T + b (``spt_skinny_linear_pre_m_f32``, (64, 13): the narrow head's forward) and
    dX = G W with the weight read transposed (``spt_skinny_linear_wt_m_f32``)."""
    from superpoint_transformer_amd import ops
    lb = L().lib
    gy, x, W, b = skinny_inputs(rows, K, N)
    assert lb.spt_skinny_linear_supported(K, N)
    both(dev, lambda put: ops._skinny_launch(put(x), put(W), put(b), mode), f"skinny forward {rows}x{K}->{N} mode {mode}")
    if N % 64:
        return
    assert lb.spt_skinny_linear_supported(N, K)

    def wt(put):
        g_, w_ = put(gy), put(W)
        y = torch.empty((rows, K), dtype=torch.float32, device=dev)
        ok(lb.spt_skinny_linear_wt_m_f32(P(g_), rows, N, P(w_), K, P(y), mode, sp(dev)), "spt_skinny_linear_wt_m_f32")
        return y

    both(dev, wt, f"skinny input gradient {rows}x{N}->{K} mode {mode}")


@pytest.mark.parametrize("mode", SKINNY_MODES)
@pytest.mark.parametrize("K,N", SKINNY)
@pytest.mark.parametrize("rows", ROWS)
def test_skinny_weight_gradient_and_one_pass_backward(rows, K, N, mode, dev):
    """dW / db (``spt_skinny_dw_pre_m_f32``), plain and with the pre-norm tables (B = 1, 3), and
    the one-pass backward (``spt_skinny_linear_bwd_m_f32``: K = 64 in the bf16 modes), plain
    and ``PRE``."""
    from superpoint_transformer_amd import ops
    lb = L().lib
    gy, x, W, _ = skinny_inputs(rows, K, N)
    assert lb.spt_skinny_dw_supported(K, N)
    both(dev, lambda put: ops._skinny_dw(put(gy), put(x), want_bias=True, mode=mode), f"skinny dW {rows} {K}x{N} mode {mode}")
    for B in (1, 3):
        if B > rows:
            continue
        am, sc, pb, batch = pre_tables(rows, K, B)

        def dw_pre(put):
            g_, x_, tabs = put(gy), put(x), [put(t) for t in (am, sc, pb, batch)]
            gw = torch.empty((N, K), dtype=torch.float32, device=dev)
            gb = torch.empty(N, dtype=torch.float32, device=dev)
            from superpoint_transformer_amd.ops import _workspace
            ws = _workspace(lb.spt_skinny_dw_workspace_bytes(K, N), dev)
            ok(lb.spt_skinny_dw_pre_m_f32(P(g_), P(x_), rows, N, K, P(gw), P(gb), *[P(t) for t in tabs], B, mode,
                                          P(ws), ws.numel(), sp(dev)), "spt_skinny_dw_pre_m_f32")
            return gw, gb

        both(dev, dw_pre, f"skinny dW PRE {rows} {K}x{N} B={B} mode {mode}")
        if not lb.spt_skinny_linear_bwd_supported(K, N, B, mode):
            assert K != 64 or mode == 0                       # what include/spt_hip.h says is built
            continue
        both(dev, lambda put: ops._skinny_bwd(put(gy), put(x), put(W), True, mode,
                                              pre=(put(am), put(sc), put(pb), put(batch), B)),
             f"one-pass backward PRE {rows} {K}x{N} B={B} mode {mode}")
    if lb.spt_skinny_linear_bwd_supported(K, N, 1, mode):
        both(dev, lambda put: ops._skinny_bwd(put(gy), put(x), put(W), True, mode),
             f"one-pass backward {rows} {K}x{N} mode {mode}")


@pytest.mark.parametrize("rows", ROWS + [4099])
def test_narrow_head_backward(rows, dev):
    """(64, 13): dX, dW and db from one pass (``spt_narrow_linear_bwd_f32``)."""
    lb = L().lib
    K, N = 64, 13
    gy, x, W, _ = skinny_inputs(rows, K, N)
    assert lb.spt_narrow_linear_bwd_supported(K, N)

    def fn(put):
        from superpoint_transformer_amd.ops import _workspace
        g_, x_, w_ = put(gy), put(x), put(W)
        gx = torch.empty((rows, K), dtype=torch.float32, device=dev)
        gw = torch.empty((N, K), dtype=torch.float32, device=dev)
        gb = torch.empty(N, dtype=torch.float32, device=dev)
        ws = _workspace(lb.spt_narrow_linear_bwd_workspace_bytes(K, N), dev)
        ok(lb.spt_narrow_linear_bwd_f32(P(g_), P(x_), P(w_), rows, N, K, P(gx), P(gw), P(gb), P(ws), ws.numel(),
                                        sp(dev)), "spt_narrow_linear_bwd_f32")
        return gx, gw, gb

    both(dev, fn, f"narrow head backward rows={rows}")


@pytest.mark.parametrize("mode", ["f32", "bf16", "f32-exact"])
@pytest.mark.parametrize("K,N", SKINNY)
@pytest.mark.parametrize("rows,B", [(r, b) for r in ROWS for b in (1, 3) if b <= r])
def test_norm_linear_and_linear_residual(rows, K, N, B, mode, dev):
    """The folded pre-norm (``spt_graphnorm_stats_f32`` + the ``PRE`` forward, its backward with
    ``spt_graphnorm_bwd_acc_f32``) and the residual epilogue, through their autograd nodes (the
    row floor of ``norm_linear_ok`` / ``linear_residual_ok`` is the callers' affair)."""
    from superpoint_transformer_amd import ops, precision
    lb = L().lib
    assert lb.spt_skinny_pre_supported(K, N, B)
    g = seeded("normlin", rows, K, N, B)
    x = torch.randn(rows, K, generator=g) * 2 + 1
    W, b = torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    gn = [1 + 0.1 * torch.randn(K, generator=g), torch.randn(K, generator=g), 1 + 0.3 * torch.randn(K, generator=g)]
    gy, gres = torch.randn(rows, N, generator=g), torch.randn(rows, K, generator=g)
    res = torch.randn(rows, N, generator=g)
    batch = sorted_batch(rows, B)

    def norm_linear(put):
        with precision.matrix_precision(mode):
            xd = put(x).requires_grad_()
            ps = [put(t).requires_grad_() for t in gn + [W, b]]
            y, xres = ops._NormLinear.apply(xd, put(batch), B, ps[0], ps[1], ps[2], 1e-5, ps[3], ps[4])
            return (y.detach(), *torch.autograd.grad([y, xres], [xd] + ps, [put(gy), put(gres)]))

    both(dev, norm_linear, f"norm_linear {rows}x{K}->{N} B={B} {mode}")
    if B > 1:
        return

    def residual(put):
        with precision.matrix_precision(mode):
            xd, r = put(x).requires_grad_(), put(res).requires_grad_()
            w_, b_ = put(W).requires_grad_(), put(b).requires_grad_()
            y = ops._ResidualLinear.apply(xd, w_, b_, r)
            return (y.detach(), *torch.autograd.grad(y, [xd, w_, b_, r], put(gy)))

    both(dev, residual, f"linear_residual {rows}x{K}->{N} {mode}")


# ---- fused MLP, fused MLP -> max-pool ------------------------------------------------------------------------------------
def mlp_layers(g, dims):
    """(W, gn weight, gn bias, gn mean scale) per layer, as CPU tensors."""
    return [(torch.randn(n, k, generator=g) * (1.5 / k ** 0.5), 1 + 0.1 * torch.randn(n, generator=g),
             0.1 * torch.randn(n, generator=g), 1 + 0.1 * torch.randn(n, generator=g))
            for k, n in zip(dims[:-1], dims[1:])]


def piecewise_batch(rows, B):
    """Three sorted thirds (the edge MLP's norm index of a B-cloud batch): 3 B runs."""
    cuts = [0, rows // 3 + 7, 2 * rows // 3 - 5, rows]
    return torch.cat([torch.arange(b - a) * B // (b - a) for a, b in zip(cuts[:-1], cuts[1:])])


@pytest.fixture(params=[1, 0, 2], ids=["bwd-split-bf16", "f32-pipe", "all-split-bf16"])
def gemm_mode(request):
    prev = L().lib.spt_fused_linear_use_split_bf16(request.param)
    yield request.param
    L().lib.spt_fused_linear_use_split_bf16(prev)


# what is built (csrc/fused_mlp.hip, csrc/fused_mlp_dma.hip): the shapes with an LDS-DMA staged backward,
# those with a pooled backward, those with bf16-stored rows, and the folded bottom layers
DMA_SHAPES = [(32, 64), (64, 128), (64, 64), (32, 32)]
POOLED_SHAPES = [(32, 64), (64, 128), (64, 64)]
STORAGE_SHAPES = [(12, 32), (32, 64), (64, 128), (64, 64)]
FOLD_SHAPES = [(12, 32, 64), (18, 32, 32)]
ST_H, ST_X, REGISTER_STAGED = 8, 16, 4              # SPT_FMLP_H_BF16 / _X_BF16 / _BWD_REGISTER_STAGED


def assert_chain_routes(dims, fold, dma, gemm_mode):
    """The backward kernels a chain of ``dims`` takes under these switches are the ones the case
    names (``spt_fused_linear_bwd_route``: 1 LDS-DMA staged, 0 register staged, -1 no fold) - a
    quiet fall-back would leave the case green without the kernel having run.  Returns whether
    the bottom layer is folded."""
    lb = L().lib
    folded = False
    if len(dims) > 2:
        r = lb.spt_fused_linear_bwd_route(dims[0], dims[1], dims[2], -1)
        # (the 12 -> 32 -> 64 fold exists as an LDS-DMA kernel only; 18 -> 32 -> 32 in both stagings)
        built = tuple(dims[:3]) in FOLD_SHAPES and gemm_mode == 1 and (bool(dma) or dims[0] == 18)
        assert (r >= 0) == built and (not built or r == dma), (dims, r, dma, gemm_mode)
        folded = fold and built
    for k, n in zip(dims[:-1], dims[1:]):
        want = int(bool(dma) and gemm_mode >= 1 and (k, n) in DMA_SHAPES)
        assert lb.spt_fused_linear_bwd_route(0, k, n, -1) == want, (k, n, dma, gemm_mode)
    return folded


CHAIN_CASES = [([12, 32, 64, 128], 1, 1), ([12, 32, 64, 128], 17, 1), ([12, 32, 64, 128], 2101, 3),
               ([18, 32, 32], 17, 1), ([18, 32, 32], 2101, -4), ([132, 64, 64], 17, 3), ([132, 64, 64], 2101, 1)]


@pytest.mark.parametrize("dma", [1, 0], ids=["dma", "registers"])
@pytest.mark.parametrize("fold", [True, False], ids=["fold", "no-fold"])
@pytest.mark.parametrize("dims,rows,B", CHAIN_CASES)
def test_fused_mlp_backward_on_flush_activations(dims, rows, B, fold, dma, gemm_mode, dev):
    """The chain's backward with everything the forward SAVED flush: the input, every raw layer
    output h_l (read as ``h`` by its own layer and as ``xprev`` by the layer above), the norm
    tables, the weights, and the upstream gradient - ``ops._fmlp_backward`` takes them as
    arguments.  This is where a short last tile's rows "meet gh = 0" (fused_mlp_dma.hip)."""
    from superpoint_transformer_amd import ops
    lb = L().lib
    g = seeded("fmlp-saved", dims, rows, B)
    batch = piecewise_batch(rows, -B) if B < 0 else sorted_batch(rows, B)
    B = abs(B)
    layers = mlp_layers(g, dims)
    x = torch.randn(rows, dims[0], generator=g) * 2 + 0.5
    gy = torch.randn(rows, dims[-1], generator=g)
    nl = len(layers)
    prev_fold, prev_dma = ops.fold_bottom(fold), lb.spt_fused_linear_bwd_use_dma(dma)
    try:
        folded = assert_chain_routes(dims, fold, dma, gemm_mode)
        with torch.cuda.device(dev):
            bd = None if batch is None else batch.to(dev)
            runs = ops.graph_runs(bd, B, rows)
            assert runs is not None and runs.B == B
            _, saved, _, _ = ops._fmlp_forward(x.to(dev), bd, runs, [1e-5] * nl, [0.01] * nl,
                                               [t.to(dev) for l in layers for t in l])
            torch.cuda.synchronize(dev)
        meta = (nl, runs, [0.01] * nl, torch.float32, not fold, -1)

        def fn(put):
            gx0, grads = ops._fmlp_backward(tuple(put(t) for t in saved), meta, put(gy))
            assert (gx0 is None) == fold
            return gx0, grads

        plain, _ = both(dev, fn, f"fused_mlp backward, flush activations {dims} rows={rows} B={B} fold={fold} dma={dma}")
        assert all(t is not None for t in plain[1]) and (not folded or plain[0] is None)
    finally:
        ops.fold_bottom(prev_fold)
        lb.spt_fused_linear_bwd_use_dma(prev_dma)


def pooled_rows(g, rows, nseg, B):
    """Rows of a sorted batch in segments numbered graph by graph (every segment has a row): the
    cuts of the graphs, ``perm`` (CSR position -> row), ``pos_seg`` and ``rowptr``."""
    cuts = [rows * b // B for b in range(B + 1)]
    seg_of_row = torch.empty(rows, dtype=torch.long)
    for b in range(B):
        lo, hi = nseg * b // B, nseg * (b + 1) // B
        assert 0 < hi - lo <= cuts[b + 1] - cuts[b]
        seg_of_row[cuts[b]:cuts[b + 1]] = torch.randint(lo, hi, (cuts[b + 1] - cuts[b],), generator=g)
        seg_of_row[cuts[b]:cuts[b] + (hi - lo)] = torch.arange(lo, hi)
    perm = torch.argsort(seg_of_row, stable=True)
    rowptr = torch.zeros(nseg + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(torch.bincount(seg_of_row, minlength=nseg), 0)
    return cuts, perm, seg_of_row[perm], rowptr


LAYER_CASES = [(k, n, pooled, store) for k, n in [(12, 32), (32, 64), (64, 128), (64, 64), (18, 32), (32, 32), (132, 64)]
               for pooled in (False, True) for store in (False, True)
               if (not pooled or ((k, n) in POOLED_SHAPES)) and (not store or (k, n) in STORAGE_SHAPES)]


@pytest.mark.parametrize("K,N,pooled,store", LAYER_CASES)
@pytest.mark.parametrize("rows,nseg,B", [(1, 1, 1), (17, 5, 1), (17, 6, 3), (2101, 90, 1), (2101, 90, 3)])
def test_fused_layer_backward_every_operand_flush(rows, nseg, B, K, N, pooled, store, dev):
    """One layer's backward at the C ABI (``spt_fused_linear_bwd_runs_f32`` /
    ``spt_fused_linear_bwd_pooled_runs_f32``, as tests/test_fused_mlp_gpu.py::
    test_bf16_storage_kernels_are_bitwise_their_f32_storage_siblings calls them) with gy - or gout,
    arg, perm, pos_seg -, h, xprev, the weight and every table flush; f32-pipe, split-bf16 and
    bf16 products, LDS-DMA and register staged, f32 and (``store``) bf16-stored rows."""
    from superpoint_transformer_amd import ops
    lb = L().lib
    assert bool(lb.spt_fused_linear_pooled_supported_ex(K, N, 1)) == ((K, N) in POOLED_SHAPES)
    assert bool(lb.spt_fused_linear_storage_supported(K, N)) == ((K, N) in STORAGE_SHAPES)
    g = seeded("fmlp-layer", rows, nseg, B, K, N)
    first = K in (12, 18, 132)                                # the chain's bottom layer: f32 input, no pre-norm
    bf = lambda t: t.to(torch.bfloat16)
    x32, h32 = torch.randn(rows, K, generator=g) * 2, torch.randn(rows, N, generator=g)
    W = torch.randn(N, K, generator=g) * 0.2
    tabK = [torch.rand(B, K, generator=g) + 0.5 for _ in range(2)] + [torch.rand(K, generator=g) + 0.5]
    tabN = [torch.rand(B, N, generator=g) + 0.5 for _ in range(2)] + [torch.rand(N, generator=g) + 0.5] + \
           [torch.rand(B, N, generator=g) + 0.5 for _ in range(3)]
    gy, gout = torch.randn(rows, N, generator=g), torch.randn(nseg, N, generator=g)
    cuts, perm, pos_seg, rowptr = pooled_rows(g, rows, nseg, B)
    off = (torch.rand(nseg, N, generator=g) * (rowptr[1:] - rowptr[:-1]).view(-1, 1)).long()
    arg = perm[rowptr[:-1].view(-1, 1) + off].int().contiguous()
    r0, r1 = (ctypes.c_int64 * B)(*cuts[:-1]), (ctypes.c_int64 * B)(*cuts[1:])
    gg = (ctypes.c_int32 * B)(*range(B))
    nbytes = lb.spt_fused_linear_workspace_bytes(K, N)

    def call(mode):
        def fn(put):
            held = []                                        # every placed operand lives until the launch is queued

            def pp(t):
                held.append(put(t))
                return P(held[-1])
            hin = put(bf(h32) if store else h32)
            xin = put(bf(x32) if (store and not first) else x32)
            w_, tn = put(W), [put(t) for t in tabN]
            pre = (None, None, None) if first else tuple(pp(t) for t in tabK)
            gx = torch.empty((rows, K), dtype=torch.float32, device=dev)
            gW = torch.empty((N, K), dtype=torch.float32, device=dev)
            prev = None if first else torch.empty((B, 2 * K + 1), dtype=torch.float64, device=dev)
            ws = ops._workspace(nbytes, dev)
            tail = (B, N, P(tn[0]), P(tn[1]), P(tn[2]), 0.01, P(tn[3]), P(tn[4]), P(tn[5]), P(xin), K, pre[0], pre[1],
                    pre[2], 0.2, P(w_), P(gx), P(gW), P(prev), mode, P(ws), ws.numel(), sp(dev))
            if pooled:
                ok(lb.spt_fused_linear_bwd_pooled_runs_f32(pp(gout), pp(arg), pp(perm.int()),
                                                           pp(pos_seg.int()), P(hin), B, r0, r1, gg, *tail),
                   "spt_fused_linear_bwd_pooled_runs_f32")
            else:
                ok(lb.spt_fused_linear_bwd_runs_f32(pp(gy), P(hin), B, r0, r1, gg, *tail),
                   "spt_fused_linear_bwd_runs_f32")
            return gx, gW, prev
        return fn

    prev_dma = lb.spt_fused_linear_bwd_use_dma(1)
    try:
        for p in ((3,) if store else (1, 3) if pooled else (0, 1, 3)):
            word = p | ((ST_H | (0 if first else ST_X)) if store else 0)
            for staged in (0, REGISTER_STAGED):
                dma = int(staged == 0 and p >= 1 and (K, N) in DMA_SHAPES and not (store and first))
                assert lb.spt_fused_linear_bwd_route(0, K, N, word | staged) == dma, (K, N, word | staged)
                both(dev, call(word | staged), f"fused layer backward {K}x{N} rows={rows} B={B} pooled={pooled} "
                                               f"mode={word | staged:#x}")
    finally:
        lb.spt_fused_linear_bwd_use_dma(prev_dma)


@pytest.mark.parametrize("mode", [1, 3, 3 | ST_X], ids=["split-bf16", "bf16", "bf16-rows"])
@pytest.mark.parametrize("K,N", POOLED_SHAPES)
@pytest.mark.parametrize("order", ["csr", "shuffled"])
@pytest.mark.parametrize("rows,nseg,B", [(1, 1, 1), (17, 5, 1), (17, 6, 3), (2101, 90, 1), (2101, 90, 3)])
def test_pool_fused_top_layer_every_operand_flush(rows, nseg, B, order, K, N, mode, dev):
    """The pool-fused top layer at the C ABI (csrc/fused_pool.hip: ``spt_fused_linear_fwd_pool_runs_f32``
    and ``spt_fused_linear_bwd_pool_runs_f32``, called as tests/fpool_harness.py calls them): the
    layer's input ``h_prev``, the CSR view, the weights and tables flush in the forward; its raw
    winners, arg positions, tables and Gram record, gout and the c tables flush in the backward."""
    lb = L().lib
    assert lb.spt_fused_linear_pool_supported(K, N, mode)
    g = seeded("fpool-abi", rows, nseg, B, K, N)
    _, seg_graph, si = pool_problem(g, rows, nseg, B)        # the first segment of every graph is empty
    if order == "csr":
        si = si.sort().values
    perm = torch.argsort(si, stable=True)
    pos_seg = si[perm].int()
    rowptr = torch.zeros(nseg + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(torch.bincount(si, minlength=nseg), 0)
    bounds = [int((seg_graph < b).sum()) for b in range(B + 1)]
    runs = [(int(rowptr[a]), int(rowptr[c]), b) for b, (a, c) in enumerate(zip(bounds[:-1], bounds[1:]))]
    n = len(runs)
    r0, r1 = (ctypes.c_int64 * n)(*[r[0] for r in runs]), (ctypes.c_int64 * n)(*[r[1] for r in runs])
    rg = (ctypes.c_int32 * n)(*[r[2] for r in runs])
    x = torch.randn(rows, K, generator=g) * 1.5 + 0.3
    if mode & ST_X:
        x = x.bfloat16()
    W = torch.randn(N, K, generator=g) * 0.1
    gnw = torch.randn(N, generator=g).abs() + 0.05
    gnw[::3] = -gnw[::3]                                     # the pool is a minimum there
    gnb, gms = torch.randn(N, generator=g) * 0.1, torch.rand(N, generator=g)
    pam, psc = torch.randn(B, K, generator=g) * 0.1, torch.rand(B, K, generator=g) + 0.5
    pbs = torch.randn(K, generator=g) * 0.1
    gout = torch.randn(nseg, N, generator=g)
    cs = [torch.randn(B, N, generator=g) * 0.1 for _ in range(3)]
    glen = int(lb.spt_fused_linear_pool_gram_len(K))
    nbytes = lb.spt_fused_linear_pool_workspace_bytes(K, N)
    f32 = dict(dtype=torch.float32, device=dev)

    def fn(put):
        from superpoint_transformer_amd.ops import _workspace
        held = []                                            # every placed operand lives until the launch is queued

        def pp(t):
            held.append(put(t))
            return P(held[-1])
        xd, pm = put(x), (None if order == "csr" else put(perm.int()))
        ps, sg = put(pos_seg), (put(seg_graph) if B > 1 else None)
        w_, b_, pa, psc_, pb_ = put(W), put(gnb), put(pam), put(psc), put(pbs)
        out, raw = torch.empty((nseg, N), **f32), torch.empty((nseg, N), **f32)
        arg, argpos = (torch.empty((nseg, N), dtype=torch.int32, device=dev) for _ in range(2))
        gram = torch.empty((B, glen), dtype=torch.float64, device=dev)
        total = torch.empty((B, 2 * N + 1), dtype=torch.float64, device=dev)
        mean, rstd, am, sc = (torch.empty((B, N), **f32) for _ in range(4))
        ws = _workspace(nbytes, dev)
        ok(lb.spt_fused_linear_fwd_pool_runs_f32(
            P(xd), P(pm), P(ps), pp(rowptr.int()), P(sg), nseg, rows, n, r0, r1, rg, B, K, P(w_), N, pp(gnw),
            P(b_), pp(gms), 1e-5, 0.01, P(pa), P(psc_), P(pb_), 0.2, P(out), P(arg), P(argpos), P(raw), P(gram),
            P(total), P(mean), P(rstd), P(am), P(sc), mode, P(ws), ws.numel(), sp(dev)), "spt_fused_linear_fwd_pool_runs_f32")
        gm = torch.empty((nseg, N), **f32)
        gx, gW = torch.empty((rows, K), **f32), torch.empty((N, K), **f32)
        ptot = torch.empty((B, 2 * K + 1), dtype=torch.float64, device=dev)
        ws = _workspace(nbytes, dev)
        ok(lb.spt_fused_linear_bwd_pool_runs_f32(
            pp(gout), pp(raw), pp(argpos), P(pm), P(ps), P(sg), nseg, n, r0, r1, rg, B, N, pp(am),
            pp(sc), P(b_), 0.01, *[pp(c) for c in cs], P(xd), K, P(pa), P(psc_), P(pb_), 0.2, P(w_),
            pp(gram), P(gm), P(gx), P(gW), P(ptot), mode, P(ws), ws.numel(), sp(dev)), "spt_fused_linear_bwd_pool_runs_f32")
        return out, arg, argpos, raw, gram, total, mean, rstd, am, sc, gm, gx, gW, ptot

    both(dev, fn, f"pool-fused top layer {K}x{N} rows={rows} B={B} {order} mode={mode:#x}")


@pytest.mark.parametrize("kind", ["f32", "raw", "bf16"])
@pytest.mark.parametrize("rows,nseg,N,B", [(1, 1, 64, 1), (17, 5, 128, 1), (17, 6, 64, 3), (2101, 90, 128, 3),
                                           (2101, 90, 64, 1), (65_536 + 19, 900, 128, 3)])
def test_segment_max_with_the_folded_norm_every_operand_flush(rows, nseg, N, B, kind, dev):
    """The materialised route's pool (``spt_segcsr_max_affine_f32``, and from 65 536 rows of 128 its
    streaming siblings with the raw output / on bf16-stored rows): the raw top-layer output
    ``h``, the CSR view, the norm tables and ``seg_graph`` flush."""
    lb = L().lib
    streaming = bool(lb.spt_segcsr_max_affine_raw_supported(N, rows))
    assert streaming == bool(lb.spt_segcsr_max_affine_bf16_supported(N, rows)) == (N == 128 and rows >= 65_536)
    if kind != "f32" and not streaming:
        return                                               # (the entry refuses: nothing to run)
    g = seeded("segmax", rows, nseg, N, B)
    _, seg_graph, si = pool_problem(g, rows, nseg, B)
    perm = torch.argsort(si, stable=True).int()
    rowptr = torch.zeros(nseg + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(torch.bincount(si, minlength=nseg), 0).int()
    h = torch.randn(rows, N, generator=g)
    if kind == "bf16":
        h = h.bfloat16()
    am, sc = torch.randn(B, N, generator=g) * 0.1, torch.randn(B, N, generator=g)    # negative scales: minima
    bs = torch.randn(N, generator=g) * 0.1

    def fn(put):
        hd, pm, rp, sg = put(h), put(perm), put(rowptr), (put(seg_graph) if B > 1 else None)
        a_, s_, b_ = put(am), put(sc), put(bs)
        out = torch.empty((nseg, N), dtype=torch.float32, device=dev)
        arg = torch.empty((nseg, N), dtype=torch.int32, device=dev)
        if kind == "raw":
            raw = torch.empty((nseg, N), dtype=torch.float32, device=dev)
            ok(lb.spt_segcsr_max_affine_raw_f32(P(hd), 0, P(pm), P(rp), rows, nseg, N, P(a_), P(s_), P(b_), 0.01, P(sg),
                                                P(out), P(arg), P(raw), sp(dev)), "spt_segcsr_max_affine_raw_f32")
            return out, arg, raw
        entry = lb.spt_segcsr_max_affine_bf16 if kind == "bf16" else lb.spt_segcsr_max_affine_f32
        ok(entry(P(hd), P(pm), P(rp), rows, nseg, N, P(a_), P(s_), P(b_), 0.01, P(sg), P(out), P(arg), sp(dev)),
           "spt_segcsr_max_affine")
        return out, arg

    both(dev, fn, f"segment max with the folded norm {rows}x{N} B={B} {kind}")


@pytest.mark.parametrize("dma", [1, 0], ids=["dma", "registers"])
@pytest.mark.parametrize("fold", [True, False], ids=["fold", "no-fold"])
@pytest.mark.parametrize("dims,rows,B", CHAIN_CASES)
def test_fused_mlp(dims, rows, B, fold, dma, gemm_mode, dev):
    """``B = -4``: the piecewise-sorted 12-run index.  ``fold``: the bottom layer's backward folded
    into the layer above (taken where the chain's input needs no gradient, so that run asks for
    none).  ``dma``: the LDS-DMA staged backward kernels against the register-staged ones."""
    from superpoint_transformer_amd import ops
    lb = L().lib
    g = seeded("fmlp", dims, rows, B)
    batch = piecewise_batch(rows, -B) if B < 0 else sorted_batch(rows, B)
    B = abs(B)
    layers = mlp_layers(g, dims)
    x = torch.randn(rows, dims[0], generator=g) * 2 + 0.5
    gy = torch.randn(rows, dims[-1], generator=g)
    prev_fold, prev_dma = ops.fold_bottom(fold), lb.spt_fused_linear_bwd_use_dma(dma)
    try:
        assert_chain_routes(dims, fold, dma, gemm_mode)

        def fn(put):
            xd = put(x)
            if not fold:
                xd.requires_grad_()
            ps = [[put(t).requires_grad_() for t in l] for l in layers]
            y = ops.fused_mlp(xd, put(batch), B, [(*l, 1e-5, 0.01) for l in ps])
            assert y is not None, "the fused route did not apply"
            wrt = ([] if fold else [xd]) + [t for l in ps for t in l]
            return (y.detach(), *torch.autograd.grad(y, wrt, put(gy)))

        both(dev, fn, f"fused_mlp {dims} rows={rows} B={B} fold={fold} dma={dma} gemm={gemm_mode}")
    finally:
        ops.fold_bottom(prev_fold)
        lb.spt_fused_linear_bwd_use_dma(prev_dma)


def pool_problem(g, rows, nseg, B):
    """A sorted batch, segments that never straddle two graphs (the first one of every graph
    stays empty where the graph has more than one), unsorted rows."""
    batch = sorted_batch(rows, B)
    seg_graph = torch.arange(nseg) * B // nseg
    si = torch.empty(rows, dtype=torch.long)
    for b in range(B):
        rmask = (batch == b) if batch is not None else torch.ones(rows, dtype=torch.bool)
        segs = torch.nonzero(seg_graph == b).flatten()
        segs = segs[1:] if segs.numel() > 1 else segs
        si[rmask] = segs[torch.randint(0, segs.numel(), (int(rmask.sum()),), generator=g)]
    return batch, seg_graph, si


@pytest.mark.parametrize("views", [False, True], ids=["index", "flush-csr"])
@pytest.mark.parametrize("precision_mode", ["f32", "bf16"])
@pytest.mark.parametrize("pool_fused", [True, False], ids=["pool-fused", "materialised"])
@pytest.mark.parametrize("dims,rows,nseg,B", [([12, 32, 64, 128], 17, 5, 1), ([12, 32, 64, 128], 2101, 90, 3),
                                              ([12, 32, 64], 2101, 90, 1),
                                              ([12, 32, 64, 128], 65_536 + 19, 900, 3)])
def test_fused_mlp_maxpool(dims, rows, nseg, B, pool_fused, precision_mode, views, dev):
    """Both routes of MLP -> max-pool with ``seg_graph``; 65 555 rows: just above the floor of the
    streaming segment-max with its raw output and, in the bf16 mode, of the bf16-stored rows."""
    from superpoint_transformer_amd import ops, precision
    g = seeded("fpool", dims, rows, nseg, B)
    batch, seg_graph, si = pool_problem(g, rows, nseg, B)
    layers = mlp_layers(g, dims)
    x = torch.randn(rows, dims[0], generator=g) * 2 + 0.5
    gout = torch.randn(nseg, dims[-1], generator=g)
    prev = ops.pool_in_forward(pool_fused)
    try:
        def fn(put):
            with precision.matrix_precision(precision_mode):
                xd = put(x).requires_grad_()
                ps = [[put(t).requires_grad_() for t in l] for l in layers]
                out = ops.fused_mlp_maxpool(xd, put(batch), B, [(*l, 1e-5, 0.01) for l in ps],
                                            segment_view(put, si, nseg, views), nseg,
                                            seg_graph=put(seg_graph))
                assert out is not None, "the fused route did not apply"
                node = out.grad_fn
                assert bool(getattr(node, "pool_fused", False)) == pool_fused
                # bf16 mode from the row floor up: the raw layer outputs are STORED as bf16
                stored = [t for t in node.saved_tensors if t is not None and t.dtype == torch.bfloat16]
                want16 = precision_mode == "bf16" and dims[-1] == 128 and rows >= 65_536
                assert bool(stored) == want16 and all(t.shape[0] == rows for t in stored)
                return (out.detach(), *torch.autograd.grad(out, [xd] + [t for l in ps for t in l], put(gout)))

        both(dev, fn, f"fused_mlp_maxpool {dims} rows={rows} B={B} fused={pool_fused} {precision_mode}")
    finally:
        ops.pool_in_forward(prev)


# ---- losses, edge affinity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS + [257])
def test_cross_entropy(rows, dev):
    from superpoint_transformer_amd import ops
    C = 13
    g = seeded("ce", rows)
    z = torch.randn(rows, C, generator=g) * 3
    target = torch.randint(0, C + 1, (rows,), generator=g)
    target[0] = 0
    w = 0.4 + 1.6 * torch.rand(C, generator=g)
    s = torch.tensor(0.37)

    for weight in (None, w):
        def fn(put):
            zd = put(z).requires_grad_()
            loss = ops.cross_entropy(zd, put(target), ignore_index=C, weight=put(weight))
            (gz,) = torch.autograd.grad(loss, zd, put(s))
            return loss.detach(), gz

        both(dev, fn, f"cross_entropy rows={rows} weighted={weight is not None}")


@pytest.mark.parametrize("mode", ["histogram", "dominant"])
@pytest.mark.parametrize("rows", ROWS + [257])
def test_histogram_loss_with_the_confusion_matrix(rows, mode, dev):
    import test_hist_loss_gpu as TH
    from superpoint_transformer_amd import ops
    C = 13
    z, h, w = (t.cpu() for t in TH.make_case(rows, C, True, dev))
    s = torch.tensor(0.37)

    def fn(put):
        zd = put(z).requires_grad_()
        cm = put(torch.zeros(C, C, dtype=torch.long))
        loss = ops.histogram_loss(zd, put(h), weight=put(w), mode=mode, confmat=cm)
        (gz,) = torch.autograd.grad(loss, zd, put(s))
        alone = ops.histogram_confusion_matrix(put(z), put(h), C)
        return loss.detach(), gz, cm, alone

    plain, _ = both(dev, fn, f"histogram_loss rows={rows} {mode}")
    expect = TH.exact_confmat(z.argmax(dim=1), h, C)
    assert torch.equal(plain[2].cpu(), expect) and torch.equal(plain[3].cpu(), expect)


@pytest.mark.parametrize("n,e,c", [(1, 1, 4), (17, 33, 8), (300, 2101, 64)])
def test_edge_affinity_features(n, e, c, dev):
    from superpoint_transformer_amd import ops
    g = seeded("affinity", n, e, c)
    x, ei = torch.randn(n, c, generator=g), torch.randint(0, n, (2, e), generator=g)
    gout = torch.randn(e, 2 * c, generator=g)

    def fn(put):
        xd = put(x).requires_grad_()
        out = ops.edge_affinity_features(xd, put(ei))
        (gx,) = torch.autograd.grad(out, xd, put(gout))
        return out.detach(), gx

    both(dev, fn, f"edge_affinity_features n={n} e={e} c={c}")


# ---- attention ------------------------------------------------------------------------------------------------------------------
def attn_graphs():
    """name -> (n, edge_index): one node with one loop; 17 nodes; the tile-boundary graphs of
    tests/test_attention_gpu.py with 361 and 9 edges and the one with edge-less nodes; 2101 nodes
    of degree ~6 with an isolated node.  Every edge count but that of the edge-less-nodes graph
    (144) is no multiple of 16."""
    import test_attention_gpu as TA
    out = {"one": (1, torch.zeros(2, 1, dtype=torch.long))}
    for name, degrees in (("17", [3, 0, 1, 16, 2, 0, 0, 5, 1, 1, 17, 1, 2, 4, 1, 0, 7]),
                          ("drift", [15, 17] * 8 + [1, 100, 1, 3]),
                          ("single", [0] * 5 + [9] + [0] * 5),
                          ("gaps", [0, 5, 0, 0, 7, 16, 0, 17, 1, 0, 31, 32, 33, 0, 2])):
        out[name] = (len(degrees), TA._degree_graph(seeded("attn-graph", name), degrees))
    g = seeded("attn-graph", 2101)
    ei = TA._rand_graph(g, 2101, 6.0)
    ei = ei[:, ei[0] != 3]
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    if ei.shape[1] % 16 == 0:
        ei = ei[:, :-1]
    out["2101"] = (2101, ei)
    for name, (n, e) in out.items():
        assert name == "gaps" or e.shape[1] % 16
    return out


LAYOUTS = {"spt64": (16, 4, 4, 32, "kqv"), "spt128-split": (16, 4, 8, 32, "kqv"), "nano-padded": (16, 2, 1, 18, "kqv"),
           "no-rpe": (8, 8, 8, 32, "")}
ROUTES = {"edge-lane-target-order": (2, 1), "edge-lane-source-order": (2, 0), "packed": (1, None), "per-node": (0, None)}


class attn_route:
    """The process switches of tests/test_attention_gpu.py::test_attention_backward_tilings_match_oracle."""

    def __init__(self, packed, target_order):
        self.packed, self.target_order = packed, target_order

    def __enter__(self):
        lb = L().lib
        self.prev = lb.spt_attn_bwd_packed(self.packed)
        self.prev_to = lb.spt_attn_bwd_el_target_order(self.target_order) if self.target_order is not None else None

    def __exit__(self, *exc):
        lb = L().lib
        lb.spt_attn_bwd_packed(self.prev)
        if self.prev_to is not None:
            lb.spt_attn_bwd_el_target_order(self.prev_to)


def attn_operands(name, layout):
    H, D, Dv, F, rpe = LAYOUTS[layout]
    n, ei = attn_graphs()[name]
    E = ei.shape[1]
    g = seeded("attn", name, layout)
    qkv = torch.randn(n, 2 * H * D + H * Dv, generator=g)
    ea = torch.randn(E, F, generator=g) * 0.5
    Ws = [(torch.randn(c, F, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1) if k in rpe else None
          for k, c in zip("kqv", (H * D, H * D, H * Dv))]
    gout = torch.randn(n, H * Dv, generator=g)
    return n, ei, qkv, ea, Ws, gout, H, D


# (without RPE the generic kernels run whatever the switches say: one route)
LAYOUT_ROUTES = [(l, r) for l in LAYOUTS for r in ROUTES if l != "no-rpe" or r == "per-node"]


@pytest.mark.parametrize("views", [False, True], ids=["edge-list", "flush-csr"])
@pytest.mark.parametrize("mode", ["f32", "bf16", "f32-exact"])
@pytest.mark.parametrize("layout,route", LAYOUT_ROUTES)
@pytest.mark.parametrize("graph", ["one", "17", "drift", "single", "gaps", "2101"])
def test_edge_attention_operands_flush(graph, layout, route, mode, views, dev):
    """``ops.edge_attention`` with qkv, edge_index (``flush-csr``: the by-source view made of it -
    row pointers, permutation, sorted targets), edge_attr, the RPE weights and the upstream
    gradient flush.  The forward has bits everywhere; the backward where no float atomics sum
    (``attention_backward_order("source")`` on the edge-lane route); the other routes are held to
    finiteness here and to their oracle in the next test - in the default precision only: in the
    bf16 and f32-exact modes the atomic routes' gradients get finiteness alone, which a NaN leak
    fails and a stray index that reads 0 does not.  (In the ``f32-exact`` mode the edge-lane
    kernels are not built: its backward sums with atomics in every order.)"""
    from superpoint_transformer_amd import ops, precision
    n, ei, qkv, ea, Ws, gout, H, D = attn_operands(graph, layout)
    packed, target_order = ROUTES[route]
    source = route == "edge-lane-source-order"
    with precision.matrix_precision(mode), precision.attention_backward_order("source" if source else None):
        word = L().lib.spt_attn_resolve_mode(precision.attention_mode())
    atomic_free = source and bool(L().lib.spt_edge_attn_bwd_el_supported(16, 4, 4, 32, word))
    assert atomic_free == (source and mode != "f32-exact")
    old_min = ops.PAD_MIN_EDGES
    if layout == "nano-padded":
        ops.PAD_MIN_EDGES = 0                          # the zero-padded route at these sizes
    try:
        with attn_route(packed, target_order):
            def fn(put):
                with precision.matrix_precision(mode), precision.attention_backward_order("source" if source else None):
                    q = put(qkv).requires_grad_()
                    e = put(ea).requires_grad_() if any(p is not None for p in Ws) else None
                    ps = [None if p is None else (put(p[0]).requires_grad_(), put(p[1]).requires_grad_()) for p in Ws]
                    out = ops.edge_attention(q, edge_view(put, ei, n, views), e, *ps, num_heads=H, qk_dim=D, scale_a=0.7)
                    wrt = [q] + ([e] if e is not None else []) + [t for p in ps if p is not None for t in p]
                    return (out.detach(), *torch.autograd.grad(out, wrt, put(gout)))

            both(dev, fn, f"edge_attention {graph} {layout} {route} {mode} views={views}",
                 bits_of=None if atomic_free else (lambda r: r[0]))
    finally:
        ops.PAD_MIN_EDGES = old_min


@pytest.mark.parametrize("route", list(ROUTES) + ["generic"])
@pytest.mark.parametrize("graph", ["17", "drift", "single", "gaps"])
def test_attention_block_flush_meets_its_oracle(graph, route, dev, monkeypatch):
    """The four backward routes in their own order (float atomics: no bits), with the block's
    input, edge list, edge features, parameters and upstream gradient flush: finite, the route
    the case names, and the f64 oracle with the bars of tests/test_attention_gpu.py::
    test_attention_backward_tilings_match_oracle.  ``generic``: 8 heads of 8 without RPE, the plain
    kernels (the layout and the oracle of ::test_edge_attention_vs_oracle)."""
    import test_attention_gpu as TA
    from oracle import spt_oracle as O
    from superpoint_transformer_amd import nn as N, ops
    routes, real_plan = [], ops._attn_bwd_plan

    def plan(*a, **k):
        routes.append(real_plan(*a, **k))
        return routes[-1]
    monkeypatch.setattr(ops, "_attn_bwd_plan", plan)
    n, ei = attn_graphs()[graph]
    E = ei.shape[1]
    g = seeded("attn-block", graph)
    rpe = route != "generic"
    H, D, dim, F = (16, 4, 64, 32) if rpe else (8, 8, 64, 32)
    blk = N.SelfAttentionBlock(dim, num_heads=H, out_dim=None, qk_dim=D, in_rpe_dim=F,
                               k_rpe=rpe, q_rpe=rpe, v_rpe=rpe)
    x = torch.randn(n, dim, generator=g)
    ea = torch.randn(E, F, generator=g) * 0.5
    gw = torch.randn(n, dim, generator=g)
    params = {k: v.detach().clone() for k, v in blk.named_parameters()}
    blk = blk.to(dev)
    packed, target_order = ROUTES[route] if rpe else (2, None)      # (2: the library's default tiling)

    def fn(put):
        for k, v in blk.named_parameters():
            v.data = put(params[k])
            v.grad = None
        xd, ead = put(x).requires_grad_(), put(ea).requires_grad_()
        out = blk(xd, put(ei), edge_attr=ead)
        wrt = [xd] + ([ead] if rpe else []) + list(blk.parameters())
        gx, *rest = torch.autograd.grad(out, wrt, put(gw))
        gea = rest.pop(0) if rpe else None
        return out.detach(), gx, gea, dict(zip([k for k, _ in blk.named_parameters()], rest))

    with attn_route(packed, target_order):
        _, (out, gx, gea, gp) = both(dev, fn, f"attention block {graph} {route}", bits_of=lambda r: r[0])
    if rpe:
        want = {(2, 1): ops.ATTN_ROUTE_EDGE_LANE_TARGET, (2, 0): ops.ATTN_ROUTE_EDGE_LANE_SOURCE,
                (1, None): ops.ATTN_ROUTE_PACKED, (0, None): ops.ATTN_ROUTE_PER_NODE}[packed, target_order]
        assert [r[0] for r in routes] == [want] * 2          # the plain and the flush run
    else:
        assert [r[0] for r in routes] == [ops.ATTN_ROUTE_VALU] * 2
    p = {k: v.double().requires_grad_() for k, v in params.items()}
    x64, ea64 = x.double().requires_grad_(), ea.double().requires_grad_()
    deg = torch.bincount(ei[0], minlength=n).double().clamp(min=1)
    old = O.qk_scale_dg
    O.qk_scale_dg = lambda s, d_, h_: ((dim // H) ** -0.5 * deg[s] ** -0.5).view(-1, 1, 1)
    try:
        ref = O.self_attention(x64, ei, ea64, p, H, D)
    finally:
        O.qk_scale_dg = old
    (ref * gw.double()).sum().backward()
    TA._check(out, ref, "out")
    TA._check(gx, x64.grad, "g_x")
    if rpe:
        TA._check(gea, ea64.grad, "g_edge_attr")
    for k in gp:
        TA._check(gp[k], p[k].grad, "g_" + k, rel_to_max=True)


@pytest.mark.parametrize("n,deg,loops", [(17, 3.0, True), (2101, 6.0, True), (700, 3.0, False)])
def test_mirror_structure_stream(n, deg, loops, dev):
    """The target-order tile records of a mirrored edge list (``spt_attn_mirror_prepare`` +
    ``spt_attn_pack_tile_ids_mirror``) from a flush edge list: integer records, bit for bit."""
    import test_attention_gpu as TA
    from superpoint_transformer_amd import csr
    ei = TA._mirrored_graph(seeded("mirror", n), n, deg, torch.device("cpu"), loops)
    pairs = ei._spt_mirror_pairs

    def fn(put):
        e = put(ei)
        e._spt_mirror_pairs = pairs
        ec = csr.edge_csr_of(e, n)
        assert ec.mirrored(1 << 6)
        rec = ec.tile_ids(1 << 6)
        assert ec._tview is None                             # the mirror route: no target view was sorted
        csr.verify_adopted(block=True)
        return ec.erowptr, ec.eperm, ec.tgt_sorted, rec

    both(dev, fn, f"mirror stream n={n}")


@pytest.mark.parametrize("G,J", [(1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("n", ROWS)
def test_attn_split_pack_and_grad(n, G, J, dev):
    lb = L().lib
    g = seeded("split", n, G, J)
    H = 16 * G
    QK, Dv, Pn = 4 * H, 4 * J, G * J
    qkv = torch.randn(n, 2 * QK + H * Dv, generator=g)
    gqa = torch.randn(Pn, n, 192, generator=g)

    def fn(put):
        q, gq = put(qkv), put(gqa)
        qa = torch.empty((Pn, n, 192), dtype=torch.float32, device=dev)
        ok(lb.spt_attn_split_pack_f32(P(q), n, G, J, P(qa), sp(dev)), "spt_attn_split_pack_f32")
        got = torch.empty((n, 2 * QK + H * Dv), dtype=torch.float32, device=dev)
        ok(lb.spt_attn_split_grad_f32(P(gq), n, G, J, P(got), sp(dev)), "spt_attn_split_grad_f32")
        return qa, got

    both(dev, fn, f"attn split pack / grad n={n} G={G} J={J}")


# =====================================================================================================
# preprocessing and transforms
# =====================================================================================================
@pytest.mark.parametrize("n,batched", [(1, False), (17, True), (2101, True), (4000, False)])
def test_voxel_groups_mean_histogram_vote_and_last(n, batched, dev):
    """``voxel_groups`` (n = 4000: two clusters 30 km apart at 3 cm, the key wider than 32 bits -
    tests/test_grid_sampling_gpu.py::test_key_wider_than_32_bits) and the reductions over its
    groups, from flush positions, features and labels."""
    import test_grid_sampling_gpu as TG
    from superpoint_transformer_amd import voxel
    size = 0.03
    pos = TG.cloud(n, size, seed=5)
    if n == 4000:
        pos[n // 2:] += torch.tensor([30_000.0, 30_000.0, 100.0])
        pos = pos[torch.randperm(n, generator=seeded("voxel-perm"))]
        coords = torch.round(pos / size).long()
        assert sum(int(c.max() - c.min()).bit_length() for c in coords.T) > 32
    g = seeded("voxel", n)
    batch = torch.randint(0, 3, (n,), generator=g) if batched else None
    x = torch.randn(n, 5, generator=g)
    normal = torch.randn(n, 3, generator=g)
    labels = TG.labels_for(n, TG.N_BINS, seed=n)

    def fn(put):
        gr = voxel.voxel_groups(put(pos), size, put(batch))
        y = put(labels)
        return (gr.pointers, gr.cluster, gr.order, gr.last, gr.coords,
                voxel.group_mean(put(x), gr), voxel.group_mean(put(normal), gr, normalize=True),
                voxel.group_mean(put(x[:, 0].contiguous()), gr),
                voxel.group_histogram(y, gr, TG.N_BINS), voxel.group_vote(y, gr), voxel.group_last(gr, seed=1234))

    plain, _ = both(dev, fn, f"voxel n={n}")
    TG.check_groups(voxel.VoxelGroups(*plain[:5], size), pos, size, batch)


def knn_cloud(n):
    g = seeded("knn-cloud", n)
    return (torch.rand(n, 3, generator=g) * torch.tensor([12.0, 9.0, 3.0])).float()


@pytest.mark.parametrize("n,k", [(1, 5), (17, 5), (2101, 12), (2101, 45)])
def test_grid_knn_with_and_without_geof(n, k, dev):
    """``knn_1`` (grid kNN; its occupancy probes run on the flush cloud too), the in-search
    eigenfeatures (``knn_1_features``, k <= 63) and the dense eigenfeatures and the density from
    the flush neighbour tables."""
    from superpoint_transformer_amd import features, neighbors as NB
    xyz = knn_cloud(n)

    def fn(put):
        p = put(xyz)
        nn, dist = NB.knn_1(p, k, r_max=2.0)
        p2 = put(xyz)
        nn2, dist2, f2 = NB.knn_1_features(p2, k, r_max=2.0, k_min=1)
        tn, td = put(nn.contiguous()), put(dist.contiguous())
        f = NB.geometric_features(put(xyz), tn, k_min=1)
        return nn.contiguous(), dist.contiguous(), nn2.contiguous(), dist2.contiguous(), f2, f, features.point_density(tn, td)

    plain, _ = both(dev, fn, f"grid kNN n={n} k={k}")
    assert torch.equal(plain[0], plain[2]) and torch.equal(plain[1], plain[3])


@pytest.mark.parametrize("n,k", [(1, 3), (17, 3), (2101, 3), (4097, 5)])
def test_neighbors_dense_to_csr_and_csr_geof(n, k, dev):
    from superpoint_transformer_amd import neighbors as NB
    g = seeded("dense", n, k)
    nn = torch.randint(0, n, (n, k), generator=g)
    nn[torch.rand(n, k, generator=g) < 0.4] = -1
    nn[-1, 0] = 0                                          # the last row is not empty
    xyz = knn_cloud(n)

    def fn(put):
        ptr, val, sizes = NB.neighbors_dense_to_csr(put(nn))
        f = NB.geometric_features_csr(put(xyz), put(val), put(ptr), k_min=1, add_self=True, raw=True)
        return ptr, val, sizes, f

    both(dev, fn, f"neighbors_dense_to_csr / csr geof n={n} k={k}")


@pytest.mark.parametrize("n", [1, 17, 2101, 4097])
def test_radius_ball(n, dev):
    lb = L().lib
    g = seeded("ball", n)
    pos = (torch.rand(n, 3, generator=g) * 10).float()
    batch = torch.randint(0, 2, (n,), generator=g)
    center = (ctypes.c_float * 3)(5.0, 4.5, 5.25)
    for cyl, use_batch in ((0, False), (1, True)):
        def fn(put):
            from superpoint_transformer_amd.ops import _workspace
            p, b = put(pos), put(batch)
            ws = _workspace(lb.spt_radius_ball_workspace_bytes(n), dev)
            out = torch.empty(n, dtype=torch.int64, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            ok(lb.spt_radius_ball_f32(P(p), n, ctypes.cast(center, ctypes.c_void_p), 6.0, cyl,
                                      P(b) if use_batch else None, 1, P(out), P(count), P(ws), ws.numel(), sp(dev)),
               "spt_radius_ball_f32")
            return out[:int(count)]

        both(dev, fn, f"radius_ball n={n} cyl={cyl}")


@pytest.mark.parametrize("n,nseg", [(1, 1), (17, 5), (2101, 300), (2101, 7)])
def test_segment_statistics_pca_and_sample(n, nseg, dev):
    """``scatter_pca``, ``scatter_std``, ``scatter_mean_orientation``, ``sparse_sample`` (with and
    without a mask) and ``segment_features`` on its draw, segments with empties."""
    from superpoint_transformer_amd import segment as S
    g = seeded("segstat", n, nseg)
    pos = knn_cloud(n)
    idx = seg_index(g, n, nseg)
    normal = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    attr = torch.randn(n, 4, generator=g)
    mask = torch.rand(n, generator=g) < 0.7

    def fn(put):
        i = put(idx)
        val, vec = S.scatter_pca(put(pos), i, nseg)
        std = S.scatter_std(put(attr), i, nseg)
        ori = S.scatter_mean_orientation(put(normal), i, nseg)
        s, ptr = S.sparse_sample(put(idx), n_max=8, n_min=2, return_pointers=True, seed=17, num_segments=nseg)
        sm, ptrm = S.sparse_sample(put(idx), n_max=8, n_min=2, mask=put(mask), return_pointers=True, seed=17,
                                   num_segments=nseg)
        feats = S.segment_features(put(pos), put(idx), nseg, samples=(put(s), put(ptr)))
        return val, vec, std, ori, s, ptr, sm, ptrm, feats

    both(dev, fn, f"segment statistics n={n} nseg={nseg}")


@pytest.mark.parametrize("n_sub,n_cl,k", [(17, 5, 3), (2101, 300, 170), (9000, 4200, 4096)])
def test_cluster_select_relabel_and_select_edges(n_sub, n_cl, k, dev):
    from oracle import spt_oracle as O
    from superpoint_transformer_amd.data import Cluster, consecutive_cluster
    lb = L().lib
    g = seeded("select", n_sub, n_cl)
    si = torch.randint(0, n_cl, (n_sub,), generator=g)
    si[:n_cl] = torch.randperm(n_cl, generator=g)
    ptr, pts = O.cluster_from_index(si, torch.arange(n_sub))
    pick = torch.randperm(n_cl, generator=g)[:k]
    E = 16 * 131 + 5
    e = torch.randint(0, n_cl, (2, E), generator=g)

    def fn(put):
        from superpoint_transformer_amd.ops import _workspace
        c2, (idx_sub, sub_super) = Cluster(put(ptr), put(pts)).select(put(pick), num_sub=n_sub)
        inv, uniq = consecutive_cluster(put(si), n_cl)
        keep = put(pick)
        table = torch.empty(n_cl, dtype=torch.int64, device=dev)
        ok(lb.spt_index_inverse(P(keep), k, n_cl, P(table), sp(dev)), "spt_index_inverse")
        de = put(e)
        ws = _workspace(lb.spt_select_edges_workspace_bytes(E), dev)
        out_e = torch.empty((2, E), dtype=torch.int64, device=dev)
        idx_e = torch.empty(E, dtype=torch.int64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        ok(lb.spt_select_edges(P(de), E, E, P(table), n_cl, P(out_e), E, P(idx_e), P(count), P(ws), ws.numel(),
                               sp(dev)), "spt_select_edges")
        kept = int(count)
        return c2.pointers, c2.points, idx_sub, sub_super, inv, uniq, out_e[:, :kept].contiguous(), idx_e[:kept]

    plain, _ = both(dev, fn, f"cluster select / relabel / select_edges n_sub={n_sub}")
    (rptr, rpts), (ridx_sub, rsub_super) = O.cluster_select(ptr, pts, pick)
    for t, r in zip(plain[:4], (rptr, rpts, ridx_sub, rsub_super)):
        assert torch.equal(t.cpu(), r)
    rinv, rperm = O.consecutive_cluster(si)
    assert torch.equal(plain[4].cpu(), rinv) and torch.equal(plain[5].cpu(), si[rperm])


@pytest.mark.parametrize("S,hi", [(17, 6), (300, 16)])
def test_cluster_graph_edges(S, hi, dev):
    from superpoint_transformer_amd import neighbors as NB
    g = seeded("clusters", S)
    sizes = torch.randint(1, hi, (S,), generator=g)
    idx = torch.repeat_interleave(torch.arange(S), sizes)
    idx = idx[torch.randperm(idx.numel(), generator=g)]
    centre = torch.rand(S, 3, generator=g) * torch.tensor([12.0, 12.0, 3.0])
    pos = (centre[idx] + (torch.rand(idx.numel(), 3, generator=g) - 0.5) * 0.6).float()

    def fn(put):
        ei, d, mid = NB.cluster_radius_nn_graph(put(pos), put(idx), 30, 0.3, None, True, 3, num_clusters=S,
                                                return_intermediate=True)
        return ei, d, mid["trimmed"], mid["anchors"], mid["center_dist"]

    both(dev, fn, f"cluster_radius_nn_graph S={S}")


@pytest.mark.parametrize("n", [1, 17, 257, 2101])
def test_partition_adjacency(n, dev):
    """Stats (+ regression), count and fill behind ``graph.partition_adjacency``, from flush
    neighbour tables and positions (tests/test_adjacency_gpu.py's synthetic tables)."""
    import adjacency_reference as R
    import test_adjacency_gpu as TAd
    from superpoint_transformer_amd.graph import partition_adjacency
    gen = seeded("adjacency", n)
    nn, dist = R.random_table(gen, n, 45)
    pos = torch.rand(n, 3, generator=gen) * 10
    r = R.partition_adjacency_reference(nn, dist, 10, 1.0, pos, 1, "mean")
    graphs = []

    def fn(put):
        gph = partition_adjacency(put(nn), put(dist), 10, w=1.0, pos=put(pos), k_isolated=1, reduce="mean")
        graphs.append(gph)
        return gph.edge_index, gph.edge_attr, gph.source_csr

    both(dev, fn, f"partition_adjacency n={n}")
    for gph in graphs:
        TAd.check_graph(gph, r, f"n = {n}")
        TAd.check_forward_star(gph, n)


@pytest.mark.parametrize("n", [65, 257, 2101])
def test_ground_bounds_trim_ransac_and_elevation(n, dev):
    import ground_reference as R
    import numpy as np
    from superpoint_transformer_amd import ground as G
    rng = np.random.default_rng(500 + n)
    pos, is_ground = R.tilted_cloud(rng, n - n // 3, n // 3, extent=30.0, origin=(1.5, -2.0))
    pos = torch.from_numpy(pos)
    vert = torch.rand(n, generator=seeded("vert", n))
    gidx = np.nonzero(is_ground)[0]
    smp = torch.from_numpy(np.stack([rng.choice(gidx, 3, replace=False) for _ in range(12)]))

    for kw in (dict(z_threshold=0.75), dict(xy_grid=0.3, z_threshold=0.75),
               dict(verticality_threshold=0.8, xy_grid=2.5)):
        def fn(put):
            p = put(pos)
            v = put(vert) if "verticality_threshold" in kw else None
            t = G.ground_mask(p, verticality=v, **kw)
            return t.indices(), t.count

        plain, _ = both(dev, fn, f"ground_mask n={n} {sorted(kw)}")
        ref = np.nonzero(R.ground_mask(pos.numpy(), verticality=vert.numpy() if "verticality_threshold" in kw else None,
                                       **kw))[0]
        assert np.array_equal(plain[0].cpu().numpy(), ref)

    def fit(put):
        p = put(pos)
        everything = G.ground_mask(p)
        # the samples index the trimmed set, which here is every point
        plane = G.fit_ground_plane(p, everything, samples=put(smp), residual_threshold=1e-3)
        return plane.counts, plane.status, G.plane_elevation(put(pos), plane, 3.0)

    both(dev, fit, f"fit_ground_plane / plane_elevation n={n}")
    both(dev, lambda put: G.ground_elevation(put(pos), z_threshold=0.75, xy_grid=0.3, random_state=3)[0],
         f"ground_elevation n={n}")


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("n", [1, 17, 257, 2101])
def test_point_colors(n, kind, dev):
    from superpoint_transformer_amd import features
    rgb = torch.randint(0, 256, (n, 3), generator=seeded("rgb", n), dtype=torch.uint8)
    rgb[0] = torch.tensor([200, 100, 50], dtype=torch.uint8)
    if kind == "f32":
        rgb = rgb.float()
    both(dev, lambda put: features.point_colors(put(rgb), ("rgb", "hsv", "lab")), f"point_colors {kind} n={n}")


@pytest.mark.parametrize("c", [1, 3, 7, 18])
@pytest.mark.parametrize("n", [1, 17, 257, 2101])
def test_augment_entries(n, c, dev):
    """The four augment entries (features, geometry in its three modes, colour range, colour),
    reading a flush tensor and writing a flush ``out``."""
    from superpoint_transformer_amd import augment as A
    g = seeded("augment", n, c)
    x = torch.randn(n, c, generator=g)
    pos, col = torch.randn(n, 3, generator=g), torch.rand(n, 3, generator=g)
    e7 = torch.randn(n, 7, generator=g)
    Rm = torch.linalg.qr(torch.randn(3, 3, generator=g)).Q
    jit = (0.02, 0.04, 99)

    def fn(put):
        res = [A.features_(put(x), jitter=jit, col_mask=A.column_mask([0]), p_rows=0.3, seed_rows=5, out=put(x * 0))]
        if c == 3:
            res += [A.geometry_(put(pos), A.POS, jitter=jit, R=Rm, scale=[1.1, 0.9, 1.0], flip_axis=1, out=put(pos * 0)),
                    A.geometry_(put(pos), A.NORMAL, R=Rm, scale=[1.1, 0.9, 1.0], flip_axis=0, out=put(pos * 0)),
                    A.geometry_(put(e7), A.EDGE7, R=Rm, scale=[1.1, 0.9, 1.0], flip_axis=2, out=put(e7 * 0)),
                    A.color_range(put(col), jit),
                    # (one row: the colour range is empty and the contrast divides 0 by 0, as it must)
                    A.color_(put(col), jitter=jit, contrast=0.5 if n > 1 else None, out=put(col * 0)),
                    A.color_(put(col), drop=True, out=put(col * 0))]
        return res

    both(dev, fn, f"augment n={n} c={c}")


def test_horizontal_and_vertical_edge_features(dev):
    """The fixtures of tests/test_transforms.py, every operand flush."""
    import test_transforms as TT
    from conftest import load_golden
    from superpoint_transformer_amd import transforms as T
    ins = TT._inputs(load_golden("horizontal_edge_features.npz"))
    for loops in (True, False):
        both(dev, lambda put: T.horizontal_edge_features(*[put(t) for t in ins], add_self_loops=loops),
             f"horizontal_edge_features loops={loops}")
    c, p = TT._vertical_inputs(load_golden("vertical_edge_features.npz"))
    both(dev, lambda put: T.vertical_edge_features({k: put(v) for k, v in c.items()}, {k: put(v) for k, v in p.items()}),
         "vertical_edge_features")


# =====================================================================================================
# everything at once
# =====================================================================================================
@pytest.mark.parametrize("clouds", [1, 3])
def test_train_steps_on_poisoned_scratch_and_fresh_tensors(clouds, dev):
    """The entries above are called one by one; the modules between them (stages, pools, the
    criterion, the optimizer's buckets) allocate with ``torch.empty`` too.  Two eager train steps of
    tests/test_capture_gpu.py's model, built and run with every workspace request cut out of a
    NaN-filled arena and every fresh floating tensor NaN-filled, in the attention backward's source
    order (bitwise reproducible: ::test_eager_step_is_bitwise_reproducible): the losses and every
    parameter afterwards are those of the ordinary run, bit for bit."""
    import test_capture_gpu as TC
    from superpoint_transformer_amd import precision
    sizes = TC.ONE_CLOUD if clouds == 1 else TC.THREE_CLOUDS
    with precision.attention_backward_order("source"):
        a = TC._path(dev, sizes)
        la = [float(a.step().detach()) for _ in range(2)]
        arena = GuardedArena(dev, guard_byte=0xFF, fill_byte=0xFF)
        with poisoned_fresh_tensors(dev):
            with exact_workspaces(arena):
                b = TC._path(dev, sizes)
                lb = [float(b.step().detach()) for _ in range(2)]
                pa, pb = TC._finish(a, b)
    assert len(arena) > 0 and la == lb and all(x == x and abs(x) != float("inf") for x in lb), (la, lb)
    all_finite(pb, "parameters after two poisoned steps")
    TC._bitwise("parameters after 2 eager steps, ordinary vs poisoned memory", TC._names(a), pb, pa)
