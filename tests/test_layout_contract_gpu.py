"""What the wrappers make of a tensor's LAYOUT: strided, offset, cast and misaligned arguments.

Every kernel takes raw pointers and indexes them by shape alone (include/spt_hip.h: row-major,
contiguous, the entry's element type, rows of whole 16-byte chunks on a 16-byte boundary).  The
Python wrappers are the only place where strides, storage offset, dtype and alignment of a
PyTorch tensor are turned into that contract (``_lib.dense``, DESIGN.md "Layout contract").  A
wrapper that forgets it reads neighbouring memory of a live allocation and returns finite,
plausible, wrong numbers.  Here every wrapper of the table runs its problem (the builders of
tests/test_flush_inputs_gpu.py, at its row counts 1 / 17 / 2101) with every floating input, every
index input, every weight and the incoming gradient in turn as

  colslice    ``wide[:, 3:3 + c]`` of an [n, c + 7] tensor; indices: ``pairs.t()`` / ``table[:, 1]``
  rowstride   ``big[::2]``
  transposed  ``xt.t()`` of a dense [c, n] tensor
  expanded    ``row.expand(n, c)`` (stride 0: what ``sum().backward()`` and broadcasts hand over)
  off4, off8  ``flat[1:1 + n c].view(n, c)`` / from ``flat[2:]``: dense, 4 / 8 bytes into a 16-byte
              line (a flat parameter or gradient buffer, a row-narrowed view of 72-byte rows);
              int64 indices: ``flat[1:1 + n]`` (8 bytes in)
  f64, bf16, int32   where the wrapper documents a cast - as every other row of a 2 n-row tensor

and asserts, per case:

  * same bits: outputs and ALL gradients equal those of the same call on ``.contiguous().clone()``
    of the view (from the allocator: aligned).  The attention runs in
    ``attention_backward_order("source")``, where nothing sums with float atomics; an f64 view's
    results, cast back, are the bits of the f32 run (f64 holds every f32 exactly);
  * inputs untouched: the skipped elements of the parent buffer are NaN (integer parents: 0) -
    a stray read shows as a NaN or a changed result - and the whole parent compares bit for bit
    with a clone taken before the call;
  * gradient form: the gradient of a view input has the view's shape and dtype;
  * once per wrapper (``off4``) the view run also meets the op's own f64 oracle at the bar of its
    own test file, so a mistake shared with the dense run cannot pass as agreement.  The helpers
    are imported from those files (``_close`` of test_segcsr_gpu / test_norms_gpu, ``bars`` of
    test_skinny_bwd_fused_gpu, ``check`` / ``closed_form`` / ``exact_confmat`` of test_hist_loss_gpu,
    ``one_ulp`` of test_panoptic_criterion_gpu, ``_check`` of test_attention_gpu,
    ``_same_features`` of test_neighbors_gpu); a bar written inside one of their tests is quoted
    with its place.  The fused MLP chains: the forward, from 100 rows up (``mlp_oracle`` says why).
    The fused routes with a predicate (``unit_sphere_assemble_ok`` / ``linear_residual_ok`` /
    ``norm_linear_ok``) are also held to the bits of the composed route, as their own tests hold
    them for dense tensors.

No pointer outside its entry's contract reaches a kernel here: the wrappers copy first, and the
C entries refuse a misaligned base on the host, ahead of their first launch (the last section:
status, message, sentinel-filled outputs untouched).  What the hardware would do with an
under-aligned 16-byte access is not probed.
"""
import ctypes
import re

import pytest
import torch

import test_flush_inputs_gpu as FI
from test_flush_inputs_gpu import L, P, seeded, sp

pytestmark = pytest.mark.gpu

ROWS = FI.ROWS                                     # 1, 17, 16 * 131 + 5

FLOAT_TAGS = ("colslice", "rowstride", "transposed", "expanded", "off4", "off8")
CAST_TAGS = ("f64", "bf16")
INDEX_TAGS = ("colslice", "rowstride", "off8", "int32")
WEIGHT_TAGS = ("off4", "transposed")
GRAD_TAGS = ("colslice", "expanded", "transposed", "off4")


def same_bits(a, b, what):
    """``same_bits`` of the guard suites on dense copies (a one-element gradient of a strided view
    keeps the view's stride, which a byte view refuses)."""
    dense = lambda r: [t.detach().clone(memory_format=torch.contiguous_format) for t in FI.flat(r)]
    FI.same_bits(dense(a), dense(b), what)


# ---- layouts ----------------------------------------------------------------------------------------
def _poison(shape, like):
    """A parent buffer whose every element is NaN (floating) or 0 (integer, bool)."""
    if like.is_floating_point():
        return torch.full(shape, float("nan"), dtype=like.dtype, device=like.device)
    return torch.zeros(shape, dtype=like.dtype, device=like.device)


def lay(t, tag):
    """(view, parent) with the values of the dense tensor ``t`` in the layout ``tag``, or None
    where the layout does not exist for this shape."""
    n = t.shape[0] if t.dim() else 1
    if tag in ("f64", "bf16", "int32"):
        dt = {"f64": torch.float64, "bf16": torch.bfloat16, "int32": torch.int32}[tag]
        if t.dim() == 0:
            v = t.to(dt)
            return v, v
        return lay(t.to(dt), "rowstride")
    if tag == "colslice":
        if t.dim() == 2 and not t.is_floating_point() and t.shape[0] == 2:       # [2, E]: pairs.t()
            parent = t.t().contiguous()
            return parent.t(), parent
        if t.dim() == 2:
            c = t.shape[1]
            parent = _poison((n, c + 7), t)
            parent[:, 3:3 + c] = t
            return parent[:, 3:3 + c], parent
        if t.dim() == 1:
            parent = _poison((n, 3), t)
            parent[:, 1] = t
            return parent[:, 1], parent
        return None
    if tag == "rowstride":
        if t.dim() == 0:
            return None
        parent = _poison((2 * n,) + tuple(t.shape[1:]), t)
        parent[::2] = t
        return parent[::2], parent
    if tag == "transposed":
        if t.dim() != 2:
            return None
        parent = t.t().contiguous()
        return parent.t(), parent
    if tag == "expanded":
        if t.dim() == 0:
            return None
        parent = t[0:1].clone()
        return parent.expand(t.shape), parent
    if tag in ("off4", "off8"):
        lead = (1 if tag == "off4" else 2) * (4 // t.element_size() if t.element_size() <= 4 else 1)
        if t.element_size() == 8:
            if tag == "off4":
                return None
            lead = 1
        parent = _poison((t.numel() + lead + 8,), t)
        parent[lead:lead + t.numel()] = t.reshape(-1)
        v = parent[lead:lead + t.numel()].view(t.shape)
        assert parent.data_ptr() % 16 == 0 and v.data_ptr() % 16 == lead * t.element_size()
        return v, parent
    raise KeyError(tag)


def tags_of(role, t):
    if role == "f":
        return FLOAT_TAGS
    if role == "fc":                                # a floating input whose wrapper documents a cast
        return FLOAT_TAGS + CAST_TAGS
    if role == "i":
        return INDEX_TAGS if t.dtype == torch.int64 else INDEX_TAGS[:3]
    if role == "i8":                                # int64 values that do not fit 32 bits
        return INDEX_TAGS[:3]
    if role == "w":
        return WEIGHT_TAGS
    if role == "g":
        return GRAD_TAGS
    return ()


class Problem:
    """``tensors``: name -> (CPU tensor, role); ``call(a)``: the wrapper on the dict of device
    tensors, returning outputs and gradients; ``oracle(a, result)``: the op's own yardstick."""

    def __init__(self, what, tensors, call, oracle=None):
        self.what, self.tensors, self.call, self.oracle = what, tensors, call, oracle


def leaf(t):
    return t.detach().requires_grad_()


def sweep(dev, prob):
    """Every tensor of the problem in every layout of its role, against the dense run."""
    base = {k: (None if t is None else t.to(dev).contiguous().clone()) for k, (t, _) in prob.tensors.items()}
    with torch.cuda.device(dev):
        dense = prob.call(dict(base))
        ran = 0
        for name, (t, role) in prob.tensors.items():
            if t is None:
                continue
            for tag in tags_of(role, t):
                made = lay(base[name], tag)
                if made is None:
                    continue
                view, parent = made
                what = f"{prob.what}: {name} as {tag}"
                assert torch.equal(view.contiguous().to(base[name].dtype), base[name]) or tag in ("bf16", "expanded"), what
                before = parent.clone()
                ref = prob.call({**base, name: view.contiguous().clone()})
                got = prob.call({**base, name: view})
                torch.cuda.synchronize(dev)
                same_bits(ref, got, what)
                same_bits(parent, before, what + " (the parent buffer)")
                if tag not in ("bf16", "expanded"):
                    # the values are those of the dense run: the same results (an f64 run's cast back)
                    cast = [r.to(d.dtype) if torch.is_tensor(r) and torch.is_tensor(d) else r
                            for r, d in zip(FI.flat(got), FI.flat(dense))]
                    same_bits(FI.flat(dense), cast, what + " (against the dense run)")
                if tag == "off4" and prob.oracle is not None:
                    prob.oracle({**base, name: view}, got)
                ran += 1
    assert ran > 0
    return dense


def test_fresh_device_tensors_pass_the_normaliser_as_they_are(dev):
    """What the hot path hands over - tensors straight from the allocator, and the slabs the
    wrappers cut out of them ([P, n, 192] passes, rows of a [2, E] index with E even) - comes back
    as the same object: no copy is added where none is needed."""
    dense = L().dense
    x = torch.randn(2101, 64, device=dev)
    assert dense(x, torch.float32) is x and dense(x) is x
    qa = torch.empty((2, 2101, 192), device=dev)
    assert dense(qa[1], torch.float32) is not None and dense(qa[1]).data_ptr() == qa[1].data_ptr()
    ei = torch.zeros((2, 2102), dtype=torch.long, device=dev)
    assert dense(ei, torch.int64, 8) is ei and dense(ei[1], torch.int64, 8).data_ptr() == ei[1].data_ptr()
    odd = torch.zeros((2, 2101), dtype=torch.long, device=dev)          # row 1 starts 8 bytes into a line
    assert dense(odd[1], torch.int64, 8).data_ptr() == odd[1].data_ptr()
    v = x[:, :32]
    d = dense(v, torch.float32)
    assert d is not v and d.is_contiguous() and d.data_ptr() % 16 == 0 and torch.equal(d, v)


def c64(t):
    return None if t is None else t.detach().cpu().double()


def lin_close(got, ref64, what):
    """A product of the tall-skinny Linear kernels against its f64 value, under the bar of their own
    file (``bars`` of tests/test_skinny_bwd_fused_gpu.py in the split-bf16 mode these run in: a
    fraction of the largest reference entry)."""
    import test_skinny_bwd_fused_gpu as TB
    bar, _ = TB.bars(0, None, None, {1: (ref64, ref64)}, 1)
    err = float((c64(got) - ref64).abs().max())
    assert got.shape == ref64.shape and err <= bar, f"{what}: max err {err:.3e}, bar {bar:.3e}"


# The GraphNorm bars of tests/test_norms_gpu.py::test_graph_norm_forward_backward, which are written
# inside that test: (forward, gradients) from 100 rows up, and for graphs of a few rows.
GN_BARS = {True: (1e-5, 2e-5), False: (1e-4, 2e-3)}


# ---- segment reductions, gathers ----------------------------------------------------------------------
SEG = {1: (1, 4), 17: (5, 7), 2101: (300, 64)}          # rows -> (segments, channels): 7 = no vector rows


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("n", ROWS)
def test_segment_reduce(n, reduce, dev):
    import test_segcsr_gpu as TS
    from oracle import spt_oracle as O
    from superpoint_transformer_amd import ops
    num_seg, c = SEG[n]
    g = seeded("layout-segred", n)
    x, idx = torch.randn(n, c, generator=g), FI.seg_index(g, n, num_seg)
    gout = torch.randn(num_seg, c, generator=g)
    want_arg = reduce == "max"

    def call(a):
        xd = leaf(a["x"])
        res = ops.segment_reduce(xd, a["idx"], num_seg, reduce, return_arg=want_arg)
        out = res[0] if want_arg else res
        (gx,) = torch.autograd.grad(out, xd, a["gout"])
        assert gx.shape == xd.shape and gx.dtype == xd.dtype
        return res, gx

    def oracle(a, got):
        x64 = a["x"].detach().cpu().double().requires_grad_()
        i = a["idx"].cpu().long()
        out = got[0][0] if want_arg else got[0]
        if want_arg:
            ref, rarg = O.scatter_max(x64, i, dim_size=num_seg)
            assert torch.equal(out.cpu().double(), ref.detach()) and torch.equal(got[0][1].cpu().long(), rarg)
        else:
            ref = O.scatter(x64, i, 0, None, num_seg, reduce)
            TS._close(out, ref.detach())
        (ref * a["gout"].cpu().double()).sum().backward()
        TS._close(got[1], x64.grad)

    sweep(dev, Problem(f"segment_reduce {reduce} {n}x{c}", {"x": (x, "fc"), "idx": (idx, "i"), "gout": (gout, "g")},
                       call, oracle))


@pytest.mark.parametrize("n,num_src,c", [(1, 1, 4), (17, 40, 7), (2101, 37, 64)])
def test_gather_rows(n, num_src, c, dev):
    from superpoint_transformer_amd import ops
    g = seeded("layout-gather", n)
    x, idx = torch.randn(num_src, c, generator=g), torch.randint(0, num_src, (n,), generator=g)
    gout = torch.randn(n, c, generator=g)

    def call(a):
        xd = leaf(a["x"])
        out = ops.gather_rows(xd, a["idx"])
        (gx,) = torch.autograd.grad(out, xd, a["gout"])
        assert gx.shape == xd.shape and gx.dtype == xd.dtype
        return out.detach(), gx

    def oracle(a, got):
        import test_segcsr_gpu as TS
        i = a["idx"].cpu().long()
        assert torch.equal(got[0].cpu(), a["x"].cpu()[i])                             # a copy: exact
        TS._close(got[1], torch.zeros(num_src, c, dtype=torch.float64).index_add_(0, i, c64(a["gout"])))

    sweep(dev, Problem(f"gather_rows {n} of {num_src}x{c}", {"x": (x, "fc"), "idx": (idx, "i"), "gout": (gout, "g")},
                       call, oracle))


@pytest.mark.parametrize("n,num_seg,c", [(1, 1, 1), (17, 5, 1), (2101, 300, 3)])
def test_segment_sum_i64(n, num_seg, c, dev):
    from superpoint_transformer_amd import ops
    g = seeded("layout-sumi64", n)
    x = torch.randint(-(1 << 40), 1 << 40, (n, c), generator=g)
    idx = FI.seg_index(g, n, num_seg)

    def oracle(a, got):
        ref = torch.zeros(num_seg, c, dtype=torch.long).index_add_(0, a["idx"].cpu().long(), a["x"].cpu().long())
        assert torch.equal(got.cpu(), ref)

    sweep(dev, Problem(f"segment_sum_i64 {n}x{c}", {"x": (x, "i8"), "idx": (idx, "i")},
                       lambda a: ops.segment_sum_i64(a["x"], a["idx"], num_seg), oracle))


@pytest.mark.parametrize("n,num_seg", [(1, 1), (17, 5), (2101, 300)])
def test_build_csr(n, num_seg, dev):
    from oracle import spt_oracle as O
    from superpoint_transformer_amd import csr
    idx = FI.seg_index(seeded("layout-csr", n), n, num_seg)

    def call(a):
        v = csr.build_csr(a["idx"], num_seg)
        return v.perm, v.rowptr, v.pos_seg()

    def oracle(a, got):
        perm, rowptr = O.csr_view(a["idx"].cpu().long(), num_seg)
        assert torch.equal(got[0].cpu(), perm) and torch.equal(got[1].cpu(), rowptr)

    sweep(dev, Problem(f"build_csr {n}/{num_seg}", {"idx": (idx, "i")}, call, oracle))


@pytest.mark.parametrize("n,e,c", [(1, 1, 4), (17, 33, 8), (300, 2101, 64)])
def test_edge_affinity_features(n, e, c, dev):
    from superpoint_transformer_amd import ops
    g = seeded("layout-affinity", n, e)
    x, ei = torch.randn(n, c, generator=g), torch.randint(0, n, (2, e), generator=g)
    gout = torch.randn(e, 2 * c, generator=g)

    def call(a):
        xd = leaf(a["x"])
        out = ops.edge_affinity_features(xd, a["ei"])
        (gx,) = torch.autograd.grad(out, xd, a["gout"])
        assert gx.shape == xd.shape and gx.dtype == xd.dtype
        return out.detach(), gx

    def oracle(a, got):
        # the forward is one rounding per element of |x_a - x_b| and (x_a + x_b) / 2: exact in f32
        xs, (s, t) = a["x"].detach().float(), a["ei"].long()
        assert torch.equal(got[0], torch.cat([(xs[s] - xs[t]).abs(), (xs[s] + xs[t]) / 2], 1))
        import test_segcsr_gpu as TS                 # the gradient ends in the segment sum: its bar
        x64, (s, t) = c64(a["x"]).requires_grad_(), a["ei"].cpu().long()
        (torch.cat([(x64[s] - x64[t]).abs(), (x64[s] + x64[t]) / 2], 1) * c64(a["gout"])).sum().backward()
        TS._close(got[1], x64.grad)

    sweep(dev, Problem(f"edge_affinity_features n={n} e={e} c={c}",
                       {"x": (x, "fc"), "ei": (ei, "i"), "gout": (gout, "g")}, call, oracle))


# ---- norms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n,nseg", [(1, 1), (17, 5), (2101, 37)])
def test_unit_sphere_norm_and_assemble(n, nseg, weighted, dev):
    import test_norms_gpu as TN
    from oracle import spt_oracle as O
    from superpoint_transformer_amd import ops
    g = seeded("layout-usn", n, nseg)
    pos = (torch.randn(n, 3, generator=g) * 5 + 20).float()
    idx = (torch.arange(n) % nseg)[torch.randperm(n, generator=g)]
    w = torch.randint(1, 300, (n,), generator=g) if weighted else None
    x = torch.randn(n, 8, generator=g)
    gout = torch.randn(n, 12, generator=g)

    def call(a):
        o, d = ops.unit_sphere_norm(a["pos"], a["idx"], a["w"], nseg)
        xd = leaf(a["x"])
        # the predicate does not look at the layout: whatever it says yes to must be right
        assert ops.unit_sphere_assemble_ok(xd, a["pos"]) == (xd.dtype == torch.float32)
        cat, d2 = ops.unit_sphere_assemble(xd, a["pos"], a["idx"], a["w"], nseg)
        (gx,) = torch.autograd.grad(cat, xd, a["gout"])
        assert gx.shape == xd.shape and gx.dtype == xd.dtype
        # the fused route against the composed one, bit for bit (tests/test_norms_gpu.py)
        ref = torch.cat([d[a["idx"].long()], o, xd.detach().float()], 1)
        assert torch.equal(cat.detach(), ref) and torch.equal(d2, d)
        assert torch.equal(gx.float(), a["gout"].float()[:, 4:])
        return o, d, cat.detach(), d2, gx

    def oracle(a, got):
        ro, rd = O.unit_sphere_norm(a["pos"].cpu().double(), a["idx"].cpu().long(),
                                    None if a["w"] is None else a["w"].cpu().long(), nseg)
        TN._close(got[0], ro)
        assert torch.equal(got[1].cpu(), rd.float())                  # f32 boxes: exact

    sweep(dev, Problem(f"unit_sphere n={n} nseg={nseg} weighted={weighted}",
                       {"pos": (pos, "fc"), "idx": (idx, "i"), "w": (w, "i"), "x": (x, "f"), "gout": (gout, "g")},
                       call, oracle))


@pytest.mark.parametrize("r,d,B,slope", [(1, 32, 1, 1.0), (17, 18, 3, 0.01), (2101, 128, 3, 0.01), (2101, 7, 1, 0.01)])
def test_graph_norm(r, d, B, slope, dev):
    import test_norms_gpu as TN
    from oracle import spt_oracle as O
    from superpoint_transformer_amd import ops
    g = seeded("layout-gn", r, d, B)
    x = (torch.randn(r, d, generator=g) * 2 + 3).float()
    batch = FI.sorted_batch(r, B)
    w, b = torch.randn(d, generator=g), torch.randn(d, generator=g)
    a_ = 1 + 0.3 * torch.randn(d, generator=g)
    gy = torch.randn(r, d, generator=g)

    def call(a):
        xd = leaf(a["x"])
        ps = [leaf(a[k]) for k in ("w", "b", "a")]
        y = ops.graph_norm(xd, a["batch"], *ps, eps=1e-5, num_graphs=B, act_slope=slope)
        grads = torch.autograd.grad(y, [xd] + ps, a["gy"])
        for t, gt in zip([xd] + ps, grads):
            assert gt.shape == t.shape
        assert grads[0].dtype == xd.dtype
        return (y.detach(), *grads)

    def oracle(a, got):
        x64 = c64(a["x"]).requires_grad_()
        p64 = [c64(a[k]).requires_grad_() for k in ("w", "b", "a")]
        ref = O.graph_norm(x64, None if B == 1 else a["batch"].cpu().long(), *p64, eps=1e-5, batch_size=B)
        gw = c64(a["gy"])
        if slope != 1.0:
            # an element within f32 rounding of the kink may take the other slope: it gets no upstream
            # gradient, in the oracle and (the same mask) in a device run of its own
            gw = gw * (ref.detach().abs() > 1e-3).double()
            ref = torch.nn.functional.leaky_relu(ref, slope)
        (ref * gw).sum().backward()
        xd = leaf(a["x"])
        ps = [leaf(a[k]) for k in ("w", "b", "a")]
        y = ops.graph_norm(xd, a["batch"], *ps, eps=1e-5, num_graphs=B, act_slope=slope)
        grads = torch.autograd.grad(y, [xd] + ps, gw.float().to(dev))
        fwd, bwd = GN_BARS[r >= 100]
        assert torch.equal(y.detach(), got[0])
        TN._close(y, ref.detach(), tol=fwd)
        for gt, rt in zip(grads, [x64] + p64):
            TN._close(gt, rt.grad, tol=bwd)

    sweep(dev, Problem(f"graph_norm {r}x{d} B={B}",
                       {"x": (x, "fc"), "batch": (batch, "i"), "w": (w, "w"), "b": (b, "w"), "a": (a_, "w"),
                        "gy": (gy, "g")}, call, oracle))


# ---- the tall-skinny Linears ---------------------------------------------------------------------------
SKINNY = {1: (64, 64), 17: (128, 128), 2101: (64, 192), 4099: (64, 192)}


@pytest.mark.parametrize("rows", ROWS)
def test_skinny_linear_kernels(rows, dev):
    """The launchers behind ``linear`` (forward, dX with the weight read transposed, dW / db, the
    one-pass backward) below the row floor of the public wrapper, as test_flush_inputs_gpu.py
    runs them."""
    from superpoint_transformer_amd import ops
    lb = L().lib
    K, N = SKINNY[rows]
    gy, x, W, b = FI.skinny_inputs(rows, K, N)
    mode = 1

    def call(a):
        y = ops._skinny_launch(a["x"], a["W"], a["b"], mode)
        gw, gb = ops._skinny_dw(a["gy"], a["x"], want_bias=True, mode=mode)
        dx = torch.empty((rows, K), dtype=torch.float32, device=dev)
        g_, w_ = L().dense(a["gy"]), L().dense(a["W"])
        FI.ok(lb.spt_skinny_linear_wt_m_f32(P(g_), rows, N, P(w_), K, P(dx), mode, sp(dev)), "spt_skinny_linear_wt_m_f32")
        res = [y, gw, gb, dx]
        if lb.spt_skinny_linear_bwd_supported(K, N, 1, mode):
            res += list(ops._skinny_bwd(a["gy"], a["x"], a["W"], True, mode))
        return res

    def oracle(a, got):
        x64, W64, b64, g64 = (c64(a[k]) for k in ("x", "W", "b", "gy"))
        refs = [x64 @ W64.t() + b64, g64.t() @ x64, g64.sum(0), g64 @ W64]
        refs += [refs[3], refs[1], refs[2]] if len(got) > 4 else []
        for i, (t, r) in enumerate(zip(got, refs)):
            lin_close(t, r, f"skinny kernels {rows} {K}->{N}: output {i}")

    sweep(dev, Problem(f"skinny kernels {rows} {K}->{N}",
                       {"x": (x, "f"), "W": (W, "w"), "b": (b, "w"), "gy": (gy, "g")}, call, oracle))


def norm_linear_f64(a, B):
    """[y, gx, g gn_weight, g gn_bias, g gn_mean_scale, gW, gb] of ``norm_linear`` in f64: the Linear
    of the GraphNorm of x, the residual branch's gradient ``gres`` joining x's."""
    from oracle import spt_oracle as O
    x64 = c64(a["x"]).requires_grad_()
    ps = [c64(a[k]).requires_grad_() for k in ("gw", "gb", "ga", "W", "b")]
    xn = O.graph_norm(x64, None if B == 1 else a["batch"].cpu().long(), ps[0], ps[1], ps[2], eps=1e-5, batch_size=B)
    y = xn @ ps[3].t() + ps[4]
    ((y * c64(a["gy"])).sum() + (x64 * c64(a["gres"])).sum()).backward()
    return [y.detach(), x64.grad] + [p.grad for p in ps]


@pytest.mark.parametrize("rows,B", [(1, 1), (17, 3), (2101, 3), (2101, 1)])
def test_norm_linear_and_linear_residual_nodes(rows, B, dev):
    from superpoint_transformer_amd import ops, precision
    K, N = SKINNY[rows]
    g = seeded("layout-normlin", rows, B)
    x = torch.randn(rows, K, generator=g) * 2 + 1
    W, b = torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    gn = [1 + 0.1 * torch.randn(K, generator=g), torch.randn(K, generator=g), 1 + 0.3 * torch.randn(K, generator=g)]
    gy, gres, res = (torch.randn(rows, N, generator=g), torch.randn(rows, K, generator=g),
                     torch.randn(rows, N, generator=g))
    batch = FI.sorted_batch(rows, B)

    def call(a):
        xd = leaf(a["x"])
        ps = [leaf(a[k]) for k in ("gw", "gb", "ga", "W", "b")]
        y, xres = ops._NormLinear.apply(xd, a["batch"], B, ps[0], ps[1], ps[2], 1e-5, ps[3], ps[4])
        out = [y.detach(), *torch.autograd.grad([y, xres], [xd] + ps, [a["gy"], a["gres"]])]
        # the folded pre-norm against linear(graph_norm(x)): the forward's bits (its own test file)
        yn = ops.graph_norm(xd.detach(), a["batch"], ps[0].detach(), ps[1].detach(), ps[2].detach(), eps=1e-5,
                            num_graphs=B)
        assert torch.equal(y.detach(), ops._skinny_launch(yn, a["W"], a["b"], precision.skinny_mode()))
        if B == 1:
            r = leaf(a["res"])
            w_, b_ = leaf(a["W"]), leaf(a["b"])
            x2 = leaf(a["x"])
            yr = ops._ResidualLinear.apply(x2, w_, b_, r)
            assert torch.equal(yr.detach(), r.detach() + ops._skinny_launch(a["x"], a["W"], a["b"],
                                                                            precision.skinny_mode()))
            out += [yr.detach(), *torch.autograd.grad(yr, [x2, w_, b_, r], a["gy"])]
        return out

    def oracle(a, got):
        what = f"norm_linear / linear_residual {rows}x{K}->{N} B={B}"
        if rows >= 100:                                  # (graphs of a few rows: see GN_BARS)
            for t, r in zip(got[:7], norm_linear_f64(a, B)):
                lin_close(t, r, what + " (norm_linear)")
        if B == 1:
            x64, W64, b64, g64 = (c64(a[k]) for k in ("x", "W", "b", "gy"))
            refs = [c64(a["res"]) + x64 @ W64.t() + b64, g64 @ W64, g64.t() @ x64, g64.sum(0), g64]
            for t, r in zip(got[7:], refs):
                lin_close(t, r, what + " (linear_residual)")

    tensors = {"x": (x, "f"), "batch": (batch, "i"), "gw": (gn[0], "w"), "gb": (gn[1], "w"), "ga": (gn[2], "w"),
               "W": (W, "w"), "b": (b, "w"), "gy": (gy, "g"), "gres": (gres, "g")}
    if B == 1:
        tensors["res"] = (res, "f")
    sweep(dev, Problem(f"norm_linear / linear_residual {rows}x{K}->{N} B={B}", tensors, call, oracle))


def test_public_linears_above_the_row_floor(dev):
    """``linear`` / ``linear_residual`` / ``norm_linear`` at 4099 rows, where their kernels run: the
    predicates say yes for every layout (they look at shape and dtype) and the fused ops give the
    bits of the composed routes."""
    from superpoint_transformer_amd import ops
    rows, B = 4099, 3
    K, N = SKINNY[rows]
    g = seeded("layout-public-linear")
    x = torch.randn(rows, K, generator=g) * 2 + 1
    W, b = torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    gn = [1 + 0.1 * torch.randn(K, generator=g), torch.randn(K, generator=g), 1 + 0.3 * torch.randn(K, generator=g)]
    res, gy = torch.randn(rows, N, generator=g), torch.randn(rows, N, generator=g)
    batch = FI.sorted_batch(rows, B)

    def call(a):
        xd, w_, b_, r = leaf(a["x"]), leaf(a["W"]), leaf(a["b"]), leaf(a["res"])
        y = ops.linear(xd, w_, b_)
        assert isinstance(y.grad_fn, ops._TallLinear._backward_cls)
        out = [y.detach(), *torch.autograd.grad(y, [xd, w_, b_], a["gy"])]
        assert ops.linear_residual_ok(r, w_)
        yr = ops.linear_residual(xd, w_, b_, r)
        assert torch.equal(yr.detach(), r.detach() + y.detach())
        out += [yr.detach(), *torch.autograd.grad(yr, [xd, w_, b_, r], a["gy"])]
        assert ops.norm_linear_ok(xd, a["batch"], B, w_)
        ps = [leaf(a[k]) for k in ("gw", "gb", "ga")]
        yn, xres = ops.norm_linear(xd, a["batch"], B, *ps, 1e-5, w_, b_)
        composed = ops.linear(ops.graph_norm(xd.detach(), a["batch"], *[p.detach() for p in ps], eps=1e-5,
                                             num_graphs=B), a["W"], a["b"])
        assert torch.equal(yn.detach(), composed)
        out += [yn.detach(), *torch.autograd.grad([yn, xres], [xd, w_, b_] + ps, [a["gy"], a["gres"]])]
        for t, gt in zip([xd, w_, b_] + ps, out[-6:]):
            assert gt.shape == t.shape and gt.dtype == t.dtype
        return out

    def oracle(a, got):
        x64, W64, b64, g64 = (c64(a[k]) for k in ("x", "W", "b", "gy"))
        lin = [x64 @ W64.t() + b64, g64 @ W64, g64.t() @ x64, g64.sum(0)]
        refs = lin + [c64(a["res"]) + lin[0]] + lin[1:] + [g64]
        n64 = norm_linear_f64(a, B)                       # [y, gx, ggw, ggb, gga, gW, gb]
        refs += [n64[0], n64[1], n64[5], n64[6], n64[2], n64[3], n64[4]]
        assert len(got) == len(refs)
        for i, (t, r) in enumerate(zip(got, refs)):
            lin_close(t, r, f"public linears: output {i}")

    gres = torch.randn(rows, K, generator=g)
    sweep(dev, Problem("linear / linear_residual / norm_linear 4099x64->192",
                       {"x": (x, "f"), "batch": (batch, "i"), "W": (W, "w"), "b": (b, "w"), "gw": (gn[0], "w"),
                        "gb": (gn[1], "w"), "ga": (gn[2], "w"), "res": (res, "f"), "gy": (gy, "g"),
                        "gres": (gres, "g")}, call, oracle))


# ---- fused MLP, fused MLP -> max-pool --------------------------------------------------------------------
def mlp_f64(a, n_layers, B):
    """The chain [bias-free Linear -> GraphNorm -> LeakyReLU(0.01)] x L in f64."""
    from oracle import spt_oracle as O
    h = c64(a["x"])
    batch = None if B == 1 else a["batch"].cpu().long()
    for i in range(n_layers):
        h = O.graph_norm(h @ c64(a[f"W{i}"]).t(), batch, *[c64(a[f"{k}{i}"]) for k in ("gw", "gb", "ga")],
                         eps=1e-5, batch_size=B)
        h = torch.nn.functional.leaky_relu(h, 0.01)
    return h


def mlp_oracle(rows, n_layers, B, pool=None):
    """The forward against the f64 chain under the GraphNorm bar the chain ends in (GN_BARS), from
    100 rows up: the bars of the chains' own files are stated for such sizes, and a graph of one or a
    few rows has (near) zero variance, where 1 / sqrt(var + eps) multiplies every rounding of the
    layer's product by up to 316 (the 1- and 17-row cases keep the bits of the dense run).  The
    gradients have no one-line yardstick: near a LeakyReLU kink an element may take either slope, and
    the three-sided oracle that judges that lives inside tests/test_fused_mlp_gpu.py."""
    def oracle(a, got):
        import test_norms_gpu as TN
        from oracle import spt_oracle as O
        if rows < 100:
            return
        ref = mlp_f64(a, n_layers, B)
        if pool is not None:
            ref, _ = O.scatter_max(ref, a["si"].cpu().long(), dim_size=pool)
        TN._close(got[0], ref, tol=GN_BARS[True][0])
    return oracle


@pytest.mark.parametrize("need_gx", [True, False], ids=["gx", "fold"])
@pytest.mark.parametrize("dims,rows,B", [([12, 32, 64, 128], 1, 1), ([12, 32, 64, 128], 17, 1),
                                         ([12, 32, 64, 128], 2101, 3), ([18, 32, 32], 2101, -4)])
def test_fused_mlp(dims, rows, B, need_gx, dev):
    """``B = -4``: the piecewise-sorted 12-run index (the edge MLP: 18 raw features, 72-byte rows).
    ``fold``: the chain's input needs no gradient, the bottom layer rides in the layer above."""
    from superpoint_transformer_amd import ops
    g = seeded("layout-fmlp", dims, rows, B)
    batch = FI.piecewise_batch(rows, -B) if B < 0 else FI.sorted_batch(rows, B)
    B = abs(B)
    layers = FI.mlp_layers(g, dims)
    x = torch.randn(rows, dims[0], generator=g) * 2 + 0.5
    gy = torch.randn(rows, dims[-1], generator=g)
    names = [f"{k}{i}" for i in range(len(layers)) for k in ("W", "gw", "gb", "ga")]

    def call(a):
        xd = leaf(a["x"]) if need_gx else a["x"].detach()
        ps = [leaf(a[k]) for k in names]
        y = ops.fused_mlp(xd, a["batch"], B, [(*ps[4 * i:4 * i + 4], 1e-5, 0.01) for i in range(len(layers))])
        assert y is not None, "the fused route did not apply"
        wrt = ([xd] if need_gx else []) + ps
        grads = torch.autograd.grad(y, wrt, a["gy"])
        for t, gt in zip(wrt, grads):
            assert gt.shape == t.shape and gt.dtype == t.dtype
        return (y.detach(), *grads)

    tensors = {"x": (x, "fc"), "batch": (batch, "i"), "gy": (gy, "g")}
    for i, l in enumerate(layers):
        for k, t in zip(("W", "gw", "gb", "ga"), l):
            tensors[f"{k}{i}"] = (t, "w")
    sweep(dev, Problem(f"fused_mlp {dims} rows={rows} B={B} need_gx={need_gx}", tensors, call,
                       mlp_oracle(rows, len(layers), B)))


@pytest.mark.parametrize("pool_fused", [True, False], ids=["pool-fused", "materialised"])
@pytest.mark.parametrize("rows,nseg,B", [(1, 1, 1), (17, 5, 1), (2101, 90, 3)])
def test_fused_mlp_maxpool(rows, nseg, B, pool_fused, dev):
    from superpoint_transformer_amd import ops
    dims = [12, 32, 64, 128]
    g = seeded("layout-fpool", rows, nseg, B)
    batch, seg_graph, si = FI.pool_problem(g, rows, nseg, B)
    layers = FI.mlp_layers(g, dims)
    x = torch.randn(rows, dims[0], generator=g) * 2 + 0.5
    gout = torch.randn(nseg, dims[-1], generator=g)
    names = [f"{k}{i}" for i in range(len(layers)) for k in ("W", "gw", "gb", "ga")]
    prev = ops.pool_in_forward(pool_fused)
    try:
        def call(a):
            xd = leaf(a["x"])
            ps = [leaf(a[k]) for k in names]
            out = ops.fused_mlp_maxpool(xd, a["batch"], B, [(*ps[4 * i:4 * i + 4], 1e-5, 0.01) for i in range(len(layers))],
                                        a["si"], nseg, seg_graph=a["seg_graph"])
            assert out is not None, "the fused route did not apply"
            assert bool(getattr(out.grad_fn, "pool_fused", False)) == pool_fused
            grads = torch.autograd.grad(out, [xd] + ps, a["gout"])
            for t, gt in zip([xd] + ps, grads):
                assert gt.shape == t.shape and gt.dtype == t.dtype
            return (out.detach(), *grads)

        tensors = {"x": (x, "fc"), "batch": (batch, "i"), "si": (si, "i"), "seg_graph": (seg_graph, "i"),
                   "gout": (gout, "g")}
        for i, l in enumerate(layers):
            for k, t in zip(("W", "gw", "gb", "ga"), l):
                tensors[f"{k}{i}"] = (t, "w")
        sweep(dev, Problem(f"fused_mlp_maxpool rows={rows} B={B} fused={pool_fused}", tensors, call,
                           mlp_oracle(rows, len(layers), B, pool=nseg)))
    finally:
        ops.pool_in_forward(prev)


@pytest.mark.parametrize("rows,B", [(17, 1), (17, 3), (2101, 3), (2101, -4)])
def test_graph_runs_and_ranges(rows, B, dev):
    """The host tables the fused layers are launched from, read off the ``batch`` argument."""
    from superpoint_transformer_amd import ops
    batch = FI.piecewise_batch(rows, -B) if B < 0 else FI.sorted_batch(rows, max(B, 2))
    nb = max(abs(B), 2)

    def call(a):
        runs = ops.graph_runs(a["batch"], nb, rows)
        ranges = ops.graph_ranges(a["batch"], nb, rows)
        return (torch.tensor([runs.r0, runs.r1, runs.g]), torch.tensor([int(runs.sorted_batch)]),
                torch.tensor(ranges if ranges is not None else [-1]))

    def oracle(a, got):
        b = a["batch"].cpu().long()
        change = torch.nonzero(b[1:] != b[:-1]).flatten() + 1
        starts = torch.cat([torch.zeros(1, dtype=torch.long), change])
        order = sorted(range(len(starts)), key=lambda i: (int(b[starts[i]]), int(starts[i])))
        assert got[0][0].tolist() == [int(starts[i]) for i in order]
        assert got[0][2].tolist() == [int(b[starts[i]]) for i in order]

    sweep(dev, Problem(f"graph_runs / graph_ranges rows={rows} B={B}", {"batch": (batch, "i")}, call, oracle))


# ---- losses ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("rows", ROWS)
def test_cross_entropy(rows, weighted, dev):
    import test_hist_loss_gpu as TH
    from superpoint_transformer_amd import ops
    C = 13
    g = seeded("layout-ce", rows)
    z = torch.randn(rows, C, generator=g) * 3
    target = torch.randint(0, C + 1, (rows,), generator=g)
    target[0] = 0
    w = (0.4 + 1.6 * torch.rand(C, generator=g)) if weighted else None
    s = torch.tensor(0.37)

    def call(a):
        zd = leaf(a["z"])
        loss = ops.cross_entropy(zd, a["target"], ignore_index=C, weight=a["w"])
        (gz,) = torch.autograd.grad(loss, zd, a["s"].to(loss.dtype))
        assert gz.shape == zd.shape and gz.dtype == zd.dtype
        return loss.detach(), gz

    def oracle(a, got):
        zd = a["z"].detach().double().requires_grad_()
        ref = torch.nn.functional.cross_entropy(zd, a["target"].long(), ignore_index=C,
                                                weight=None if a["w"] is None else a["w"].double())
        (ref * a["s"].double()).backward()
        TH.check(got[0], got[1], ref.detach(), zd.grad)

    sweep(dev, Problem(f"cross_entropy rows={rows} weighted={weighted}",
                       {"z": (z, "fc"), "target": (target, "i"), "w": (w, "w"), "s": (s, "g")}, call, oracle))


@pytest.mark.parametrize("mode", ["histogram", "dominant"])
@pytest.mark.parametrize("rows", ROWS)
def test_histogram_loss_and_confusion_matrix(rows, mode, dev):
    import test_hist_loss_gpu as TH
    from superpoint_transformer_amd import ops
    C = 13
    z, h, w = (t.cpu() for t in TH.make_case(rows, C, True, dev))
    s = torch.tensor(0.37)

    def call(a):
        zd = leaf(a["z"])
        cm = torch.zeros(C, C, dtype=torch.long, device=dev)
        loss = ops.histogram_loss(zd, a["h"], weight=a["w"], mode=mode, confmat=cm)
        (gz,) = torch.autograd.grad(loss, zd, a["s"].to(loss.dtype))
        assert gz.shape == zd.shape and gz.dtype == zd.dtype
        alone = ops.histogram_confusion_matrix(a["z"], a["h"], C)
        labels = ops.histogram_confusion_matrix(a["z"].argmax(dim=1), a["h"], C)
        return loss.detach(), gz, cm, alone, labels

    def oracle(a, got):
        zd = a["z"].detach().double().requires_grad_()
        ref = TH.closed_form(zd, a["h"].long(), a["w"].double(), mode)
        (ref * a["s"].double()).backward()
        TH.check(got[0], got[1], ref.detach(), zd.grad)
        expect = TH.exact_confmat(a["z"].cpu().argmax(dim=1), a["h"].cpu().long(), C)
        assert all(torch.equal(m.cpu(), expect) for m in got[2:])

    sweep(dev, Problem(f"histogram_loss rows={rows} {mode}",
                       {"z": (z, "fc"), "h": (h, "i"), "w": (w, "w"), "s": (s, "g")}, call, oracle))


@pytest.mark.parametrize("e", ROWS)
def test_edge_affinity_loss(e, dev):
    from superpoint_transformer_amd import ops
    g = seeded("layout-eal", e)
    n = max(2, e // 3)
    logits, target = torch.randn(e, generator=g) * 2, torch.rand(e, generator=g)
    ei = torch.randint(0, n, (2, e), generator=g)
    void = torch.rand(n, generator=g) < 0.2
    void[ei[0, 0]] = False                                  # one kept edge at least
    obj, y = torch.randint(0, 5, (n,), generator=g), torch.randint(0, 3, (n,), generator=g)
    s = torch.tensor(0.37)

    def call(a, where=None):
        x = leaf(a["logits"])
        stats = torch.zeros(4, dtype=torch.int64, device=where or dev)
        loss = ops.edge_affinity_loss(x, a["target"], a["ei"], a["void"], a["obj"], a["y"],
                                      case_weights=[0.5, 4.0, 1.0, 2.0], pos_weight=2.5, stats=stats)
        (gx,) = torch.autograd.grad(loss, x, a["s"].to(loss.dtype))
        assert gx.shape == x.shape and gx.dtype == x.dtype
        return loss.detach(), gx, stats

    def oracle(a, got):
        # the CPU route of the same rules (f64 terms, one rounding), as the op's own file holds it
        import test_panoptic_criterion_gpu as TPC
        ref = call({k: v.detach().cpu().contiguous() for k, v in a.items()}, where="cpu")
        TPC.one_ulp(got[0], ref[0], f"edge_affinity_loss e={e}: loss")
        TPC.one_ulp(got[1], ref[1], f"edge_affinity_loss e={e}: gradient")
        assert torch.equal(got[2].cpu(), ref[2])

    sweep(dev, Problem(f"edge_affinity_loss e={e}",
                       {"logits": (logits, "fc"), "target": (target, "fc"), "ei": (ei, "i"), "void": (void, "i"),
                        "obj": (obj, "i"), "y": (y, "i"), "s": (s, "g")}, call, oracle))


# ---- attention ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["spt64", "spt128-split", "no-rpe"])
@pytest.mark.parametrize("graph", ["one", "17", "2101"])
def test_edge_attention(graph, layout, dev):
    """In ``attention_backward_order("source")``: the edge-lane backward sums without atomics, so
    every gradient has bits (the generic kernels of ``no-rpe`` sum dk / dv with atomics: the forward
    and the dq columns of the qkv gradient only).  Operands as tests/test_attention_gpu.py::
    test_edge_attention_vs_oracle builds them - a ``SelfAttentionBlock`` of default initialisation,
    qkv = its Linear of random rows, its RPE encoders' parameters, its qk scale - on the graphs of the
    guard suite; oracle: ``spt_oracle.self_attention`` with an identity qkv Linear and no out_proj
    (the op itself) under that file's ``_check``."""
    from superpoint_transformer_amd import nn as N, ops, precision
    H, D, Dv, F, kinds = FI.LAYOUTS[layout]
    n, ei = FI.attn_graphs()[graph]
    rpe, dim = bool(kinds), H * Dv
    g = seeded("layout-attn", graph, layout)
    torch.manual_seed(int(g.initial_seed()) % (1 << 31))
    blk = N.SelfAttentionBlock(dim, num_heads=H, out_dim=None, qk_dim=D, in_rpe_dim=F, k_rpe=rpe, q_rpe=rpe, v_rpe=rpe)
    with torch.no_grad():
        qkv = blk.qkv(torch.randn(n, dim, generator=g)).clone()
    ea = torch.randn(ei.shape[1], F, generator=g) * 0.5
    gout = torch.randn(n, dim, generator=g)
    pr = {k_: v.detach().clone() for k_, v in blk.named_parameters()}
    Ws = [(pr[f"{k_}_rpe.weight"], pr[f"{k_}_rpe.bias"]) if rpe else None for k_ in "kqv"]
    scale_a = (dim // H) ** -0.5                      # qk_scale=None: (dim / heads)^-0.5 deg^-0.5
    tensors = {"qkv": (qkv, "fc"), "ei": (ei, "i"), "gout": (gout, "g")}
    if rpe:
        tensors["ea"] = (ea, "fc")
        for k, p in zip("kqv", Ws):
            tensors["W" + k], tensors["b" + k] = (p[0], "w"), (p[1], "w")

    def call(a):
        with FI.attn_route(2, 0), precision.attention_backward_order("source"):
            q = leaf(a["qkv"])
            e = leaf(a["ea"]) if rpe else None
            ps = [(leaf(a["W" + k]), leaf(a["b" + k])) if rpe else None for k in "kqv"]
            out = ops.edge_attention(q, a["ei"], e, *ps, num_heads=H, qk_dim=D, scale_a=scale_a)
            wrt = [q] + ([e] if rpe else []) + [t for p in ps if p is not None for t in p]
            grads = torch.autograd.grad(out, wrt, a["gout"])
            for t, gt in zip(wrt, grads):
                assert gt.shape == t.shape and gt.dtype == t.dtype
            return (out.detach(), *grads) if rpe else (out.detach(), grads[0][:, :H * D])

    def oracle(a, got):
        import test_attention_gpu as TA
        from oracle import spt_oracle as O
        q64 = c64(a["qkv"]).requires_grad_()
        e64 = c64(a["ea"]).requires_grad_() if rpe else None
        e_i = a["ei"].cpu().long()
        p = {"qkv.weight": torch.eye(q64.shape[1], dtype=torch.float64)}
        if rpe:
            for k in "kqv":
                p[f"{k}_rpe.weight"] = c64(a["W" + k]).requires_grad_()
                p[f"{k}_rpe.bias"] = c64(a["b" + k]).requires_grad_()
        deg = torch.bincount(e_i[0], minlength=n).double().clamp(min=1)
        old = O.qk_scale_dg
        O.qk_scale_dg = lambda s_, d_, h_: (scale_a * deg[s_] ** -0.5).view(-1, 1, 1)     # scale_mode 0
        try:
            ref = O.self_attention(q64, e_i, e64, p, H, D)
        finally:
            O.qk_scale_dg = old
        (ref * c64(a["gout"])).sum().backward()
        what = f"edge_attention {graph} {layout}"
        TA._check(got[0], ref, what + " out")
        if not rpe:
            TA._check(got[1], q64.grad[:, :H * D], what + " dq")
            return
        TA._check(got[1], q64.grad, what + " g_qkv")
        TA._check(got[2], e64.grad, what + " g_edge_attr")
        for i, k in enumerate("kqv"):
            TA._check(got[3 + 2 * i], p[f"{k}_rpe.weight"].grad, what + f" g_W{k}", rel_to_max=True)
            TA._check(got[4 + 2 * i], p[f"{k}_rpe.bias"].grad, what + f" g_b{k}", rel_to_max=True)

    sweep(dev, Problem(f"edge_attention {graph} {layout}", tensors, call, oracle))


# ---- segment statistics, neighbours --------------------------------------------------------------------------
@pytest.mark.parametrize("n,nseg", [(1, 1), (17, 5), (2101, 300)])
def test_segment_statistics_and_sample(n, nseg, dev):
    from superpoint_transformer_amd import segment as S
    g = seeded("layout-segstat", n, nseg)
    pos, idx = FI.knn_cloud(n), FI.seg_index(g, n, nseg)
    normal = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    attr = torch.randn(n, 4, generator=g)
    mask = torch.rand(n, generator=g) < 0.7

    def call(a):
        val, vec = S.scatter_pca(a["pos"], a["idx"], nseg)
        std = S.scatter_std(a["attr"], a["idx"], nseg)
        ori = S.scatter_mean_orientation(a["normal"], a["idx"], nseg)
        s, ptr = S.sparse_sample(a["idx"], n_max=8, n_min=2, return_pointers=True, seed=17, num_segments=nseg)
        sm, ptrm = S.sparse_sample(a["idx"], n_max=8, n_min=2, mask=a["mask"], return_pointers=True, seed=17,
                                   num_segments=nseg)
        return val, vec, std, ori, s, ptr, sm, ptrm

    def oracle(a, got):
        """``scatter_std`` at the bar of tests/test_segment_gpu.py::test_scatter_std_matches_the_f64_oracle
        (written inside it: allclose 1e-5 / 1e-5), the eigenvalues and the mean orientation under the
        segment kernels' ``_close``; the sampler by its contract: a draw of between n_min and n_max
        distinct elements of every segment (all of a smaller one), grouped by segment, masked
        elements never drawn (how many of a segment smaller than n_min: the sampler's own tests)."""
        import test_segcsr_gpu as TS
        from oracle import spt_oracle as O
        i = a["idx"].cpu().long()
        val, vec, std, ori, s_, ptr, sm, ptrm = got
        assert torch.allclose(c64(std), O.scatter_std(c64(a["attr"]), i, 0, None, nseg), atol=1e-5, rtol=1e-5)
        rv, _ = O.scatter_pca(c64(a["pos"]), i, nseg)
        TS._close(val, rv)
        TS._close(ori, O.scatter_mean_orientation(c64(a["normal"]), i, nseg))
        for smp, pt, ok in ((s_.cpu(), ptr.cpu(), torch.ones(n, dtype=torch.bool)), (sm.cpu(), ptrm.cpu(), a["mask"].cpu())):
            cnt = pt[1:] - pt[:-1]
            assert int(pt[0]) == 0 and int(pt[-1]) == smp.numel() and bool((cnt <= 8).all())
            assert torch.equal(i[smp], torch.repeat_interleave(torch.arange(nseg), cnt)) and bool(ok[smp].all())

    sweep(dev, Problem(f"segment statistics n={n} nseg={nseg}",
                       {"pos": (pos, "fc"), "idx": (idx, "i"), "normal": (normal, "fc"), "attr": (attr, "fc"),
                        "mask": (mask, "i")}, call, oracle))


@pytest.mark.parametrize("n,k", [(1, 5), (17, 5), (2101, 12)])
def test_neighbour_searches_and_features(n, k, dev):
    from superpoint_transformer_amd import neighbors as NB
    xyz = FI.knn_cloud(n)
    query = FI.knn_cloud(n + 3)[: max(1, n // 2)]
    nn = torch.randint(0, n, (n, k), generator=seeded("layout-nn", n))
    nn[torch.rand(n, k, generator=seeded("layout-nn-miss", n)) < 0.4] = -1
    nn[-1, 0] = 0

    def call(a):
        i, d = NB.frnn_grid_points(a["query"], a["xyz"], k, 2.0)
        i2, d2, f2 = NB.knn_1_features(a["xyz"], k, r_max=2.0, k_min=1)
        f = NB.geometric_features(a["xyz"], a["nn"], k_min=1, order=False)
        ptr, val, sizes = NB.neighbors_dense_to_csr(a["nn"])
        return i.contiguous(), d.contiguous(), i2.contiguous(), d2.contiguous(), f2, f, ptr, val, sizes

    def oracle(a, got):
        """The searches against the exhaustive f32 twin of the oracle (exact, as in
        tests/test_neighbors_gpu.py), the CSR against its rule, the in-search features against
        ``geometric_features`` on the stored rows under ``_same_features`` of that file."""
        import test_neighbors_gpu as TNB
        from oracle import spt_oracle as O
        d, i, i2, d2, f2, f, ptr, val, sizes = got
        pts, q = a["xyz"].detach().cpu().float(), a["query"].detach().cpu().float()
        rd, ri = O.frnn_grid_points(q, pts, k, 2.0)
        assert torch.equal(i.cpu(), ri) and torch.equal(d.cpu(), rd)
        rp, rv, rs = O.neighbors_dense_to_csr(a["nn"].cpu().long())
        assert torch.equal(ptr.cpu(), rp) and torch.equal(val.cpu(), rv) and torch.equal(sizes.cpu(), rs)
        if n >= 100:
            f0 = NB.geometric_features(a["xyz"], i2, k_min=1, order=False)
            TNB._same_features(f2, f0, pts, i2.cpu(), f"neighbours n={n} k={k}")

    sweep(dev, Problem(f"neighbours n={n} k={k}", {"xyz": (xyz, "fc"), "query": (query, "fc"), "nn": (nn, "i")}, call,
                       oracle))


# ---- the host-side refusals of the C ABI -----------------------------------------------------------------------
SENTINEL = -1234.5


def _refused(st, arg, outputs):
    """A non-zero status, the argument named in the error text, every output still the sentinel."""
    assert st != 0, f"a misaligned {arg} was accepted"
    msg = L().last_error()
    assert "aligned" in msg and re.search(rf"[ :/]{re.escape(arg)}( /| must)", msg), (arg, msg)
    torch.cuda.synchronize()
    for o in outputs:
        assert bool((o == (SENTINEL if o.is_floating_point() else -77)).all()), f"{arg}: an output was written"


def _buf(dev, numel, dtype=torch.float32):
    """A sentinel-filled buffer with 8 spare elements, so that ``ptr + 4`` stays inside it."""
    return torch.full((numel + 8,), SENTINEL if dtype.is_floating_point else -77, dtype=dtype, device=dev)


REFUSALS = ["segcsr_reduce", "segcsr_reduce_bwd", "gather_rows", "segcsr_max_affine", "graphnorm_fwd",
            "graphnorm_stats", "graphnorm_bwd_acc", "graphnorm_apply", "graphnorm_bwd_stats",
            "edge_affinity_features", "edge_affinity_features_bwd", "unit_sphere_assemble", "attn_split",
            "skinny_linear", "skinny_linear_wt", "skinny_dw", "skinny_linear_bwd", "fused_linear_fwd",
            "fused_linear_bwd", "fused_linear_bwd_fold", "fused_linear_bwd_pooled", "fused_linear_fwd_pool", "fused_linear_bwd_pool",
            "segcsr_max_affine_stream", "edge_attn_fwd", "edge_attn_bwd"]


@pytest.mark.parametrize("entry", REFUSALS)
def test_misaligned_pointers_are_refused_on_the_host(entry, dev):
    """Each entry with ``ptr + 4`` for one 16-byte-aligned argument after the other.  The refusal is
    an ``SPT_CHECK_ARG`` that stands with the entry's other argument checks, ahead of its first
    launch and its first ``hipMemsetAsync``, so nothing runs on the bad pointer: the status is
    non-zero, ``spt_last_error`` names the argument and no output changes."""
    from superpoint_transformer_amd import ops
    lb, s = L().lib, sp(dev)
    n, c, S, B = 32, 8, 4, 1
    f = lambda numel: _buf(dev, numel)
    i32 = lambda numel: _buf(dev, numel, torch.int32)
    x, out, gx, gy, y = f(n * c), f(S * c), f(n * c), f(n * c), f(n * c)
    arg = i32(S * c)
    perm = torch.arange(n, dtype=torch.int32, device=dev)
    rowptr = torch.arange(0, n + 1, n // S, dtype=torch.int32, device=dev)
    idx = (torch.arange(n, device=dev) // (n // S)).long()
    tab = [torch.ones(max(c, 256), device=dev) for _ in range(8)]
    ws = ops._workspace(1 << 20, dev)
    outs = [out, gx, y, arg]

    def each(names, fn):
        """``fn(off)`` with ``off[name] = 4`` for one name at a time."""
        for nm in names:
            st = fn({k: (4 if k == nm else 0) for k in names})
            _refused(st, nm, outs)

    if entry == "segcsr_reduce":
        each(["x", "out", "arg"], lambda o: lb.spt_segcsr_reduce_f32(
            3, P(x) + o["x"], P(perm), P(rowptr), n, S, c, P(out) + o["out"], P(arg) + o["arg"], s))
    elif entry == "segcsr_reduce_bwd":
        each(["gout", "gx"], lambda o: lb.spt_segcsr_reduce_bwd_f32(
            0, P(out) + o["gout"], None, P(idx), P(perm), P(rowptr), n, S, c, P(gx) + o["gx"], s))
    elif entry == "gather_rows":
        each(["x", "out"], lambda o: lb.spt_gather_rows_f32(P(x) + o["x"], P(idx), n, n, c, P(gx) + o["out"], s))
    elif entry == "segcsr_max_affine":
        each(["x", "out", "arg"], lambda o: lb.spt_segcsr_max_affine_f32(
            P(x) + o["x"], P(perm), P(rowptr), n, S, c, P(tab[0]), P(tab[1]), P(tab[2]), 0.01, None,
            P(out) + o["out"], P(arg) + o["arg"], s))
    elif entry == "graphnorm_fwd":
        each(["x", "y"], lambda o: lb.spt_graphnorm_fwd_f32(
            P(x) + o["x"], None, n, c, B, P(tab[0]), P(tab[1]), P(tab[2]), 1e-5, 1.0, P(y) + o["y"], P(tab[3]),
            P(tab[4]), P(ws), ws.numel(), s))
    elif entry == "graphnorm_stats":
        each(["x"], lambda o: lb.spt_graphnorm_stats_f32(
            P(x) + o["x"], None, n, c, B, P(tab[0]), P(tab[1]), 1e-5, P(tab[2]), P(tab[3]), P(tab[4]), P(tab[5]),
            P(ws), ws.numel(), s))
    elif entry == "graphnorm_bwd_acc":
        each(["x", "gy", "gx_add", "gx"], lambda o: lb.spt_graphnorm_bwd_acc_f32(
            P(x) + o["x"], P(gy) + o["gy"], None, n, c, B, P(tab[0]), P(tab[1]), P(tab[2]), P(tab[3]), P(tab[4]), 1.0,
            P(y) + o["gx_add"], P(gx) + o["gx"], P(tab[5]), P(tab[6]), P(tab[7]), P(ws), ws.numel(), s))
    elif entry == "graphnorm_apply":
        each(["x", "y"], lambda o: lb.spt_graphnorm_apply_f32(
            P(x) + o["x"], None, n, c, B, P(tab[0]), P(tab[1]), P(tab[2]), 1.0, P(y) + o["y"], s))
    elif entry == "graphnorm_bwd_stats":
        total = torch.full((B, 2 * c + 1), SENTINEL, dtype=torch.float64, device=dev)
        outs.append(total)
        each(["x", "gy"], lambda o: lb.spt_graphnorm_bwd_stats_f32(
            P(x) + o["x"], P(gy) + o["gy"], None, n, c, B, P(tab[0]), P(tab[1]), P(tab[2]), 1.0, P(total), P(ws),
            ws.numel(), s))
    elif entry == "edge_affinity_features":
        o2 = f(n * 2 * c)
        outs.append(o2)
        each(["x", "out"], lambda o: lb.spt_edge_affinity_features_f32(
            P(x) + o["x"], n, c, P(idx), P(idx), n, P(o2) + o["out"], s))
    elif entry == "edge_affinity_features_bwd":
        go, gend = f(n * 2 * c), f(2 * n * c)
        outs.append(gend)
        each(["x", "gout", "gend"], lambda o: lb.spt_edge_affinity_features_bwd_f32(
            P(x) + o["x"], P(go) + o["gout"], n, c, P(idx), P(idx), n, P(gend) + o["gend"], s))
    elif entry == "unit_sphere_assemble":
        pos, cat = torch.rand(n, 3, device=dev), f(n * (4 + c))
        diam, center = torch.full((S,), SENTINEL, device=dev), torch.full((S, 3), SENTINEL, device=dev)
        outs += [cat, diam, center]
        each(["x", "xcat"], lambda o: lb.spt_unit_sphere_assemble_ws_f32(
            P(pos), P(idx), P(perm), P(rowptr), None, None, n, S, P(x) + o["x"], c, P(cat) + o["xcat"], P(diam),
            P(center), P(ws), ws.numel(), s))
    elif entry == "attn_split":
        q, qa = f(n * 320), f(2 * n * 192)
        outs += [qa]
        each(["qkv", "qa"], lambda o: lb.spt_attn_split_pack_f32(P(q) + o["qkv"], n, 1, 2, P(qa) + o["qa"], s))
        gq = f(n * 256)
        outs += [gq]
        each(["gqa", "gqkv"], lambda o: lb.spt_attn_split_grad_f32(P(qa) + o["gqa"], n, 1, 2, P(gq) + o["gqkv"], s))
    elif entry in ("skinny_linear", "skinny_linear_wt", "skinny_dw", "skinny_linear_bwd"):
        K, N = 64, 64
        xs, W, ys, gys = f(n * K), f(N * K), f(n * N), f(n * N)
        gw, gb, gxs = f(N * K), f(N), f(n * K)
        outs += [ys, gw, gb, gxs]
        if entry == "skinny_linear":
            each(["x", "W"], lambda o: lb.spt_skinny_linear_pre_m_f32(
                P(xs) + o["x"], n, K, P(W) + o["W"], None, N, P(ys), None, None, None, None, 1, None, 1, s))
        elif entry == "skinny_linear_wt":
            each(["x", "Wt"], lambda o: lb.spt_skinny_linear_wt_m_f32(
                P(gys) + o["x"], n, N, P(W) + o["Wt"], K, P(gxs), 1, s))
        elif entry == "skinny_dw":
            each(["gy", "x"], lambda o: lb.spt_skinny_dw_pre_m_f32(
                P(gys) + o["gy"], P(xs) + o["x"], n, N, K, P(gw), P(gb), None, None, None, None, 1, 1, P(ws),
                ws.numel(), s))
        else:
            assert lb.spt_skinny_linear_bwd_supported(K, N, 1, 1)
            each(["gy", "x"], lambda o: lb.spt_skinny_linear_bwd_m_f32(
                P(gys) + o["gy"], P(xs) + o["x"], P(W), n, N, K, P(gxs), P(gw), P(gb), None, None, None, None, 1, 1,
                P(ws), ws.numel(), s))
    elif entry in ("fused_linear_fwd", "fused_linear_bwd"):
        K, N = 32, 64
        r0, r1, rg = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(n), (ctypes.c_int32 * 1)(0)
        xs, W, h, gys, gxs, gW = f(n * K), f(N * K), f(n * N), f(n * N), f(n * K), f(N * K)
        total = torch.full((1, 2 * N + 1), SENTINEL, dtype=torch.float64, device=dev)
        outs += [h, total, gxs, gW]
        if entry == "fused_linear_fwd":
            each(["x", "W", "h"], lambda o: lb.spt_fused_linear_fwd_runs_f32(
                P(xs) + o["x"], 1, r0, r1, rg, 1, K, P(W) + o["W"], N, None, None, None, 1.0, P(h) + o["h"],
                P(total), -1, P(ws), ws.numel(), s))
        else:
            each(["gy", "h", "xprev", "W", "gx"], lambda o: lb.spt_fused_linear_bwd_runs_f32(
                P(gys) + o["gy"], P(h) + o["h"], 1, r0, r1, rg, 1, N, P(tab[0]), P(tab[1]), P(tab[2]), 0.01,
                P(tab[3]), P(tab[4]), P(tab[5]), P(xs) + o["xprev"], K, None, None, None, 1.0, P(W) + o["W"],
                P(gxs) + o["gx"], P(gW), None, -1, P(ws), ws.numel(), s))
    elif entry == "fused_linear_bwd_fold":
        # the bottom layer 12 -> 32 folded into the backward of 32 -> 64: x0, W0 and gW0 [32, 12]
        K0, K, N = 12, 32, 64
        assert lb.spt_fused_linear_bwd_fold_supported(K0, K, N, -1)
        r0, r1, rg = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(n), (ctypes.c_int32 * 1)(0)
        gys, h, xs, W, gW = f(n * N), f(n * N), f(n * K), f(N * K), f(N * K)
        x0, W0, gW0 = f(n * K0), f(K * K0), f(K * K0)
        pn = L().GnBwdTables(*[P(t) for t in tab[:4]], *[P(f(256)) for _ in range(6)])
        outs += [gW, gW0]
        each(["fold_x0", "fold_W0", "fold_gW0"], lambda o: lb.spt_fused_linear_bwd_runs_gn_fold_f32(
            P(gys), P(h), 1, r0, r1, rg, 1, N, P(tab[0]), P(tab[1]), P(tab[2]), 0.01, P(tab[3]), P(tab[4]), P(tab[5]),
            P(xs), K, P(tab[6]), P(tab[7]), P(tab[0]), 0.01, P(W), P(gW), -1, P(ws), ws.numel(), ctypes.addressof(pn),
            P(x0) + o["fold_x0"], K0, P(W0) + o["fold_W0"], P(gW0) + o["fold_gW0"], s))
    elif entry in ("fused_linear_bwd_pooled", "fused_linear_fwd_pool", "fused_linear_bwd_pool"):
        from superpoint_transformer_amd import precision
        K, N = 64, 128
        r0, r1, rg = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(n), (ctypes.c_int32 * 1)(0)
        xs, W, h, gxs, gW, gm = f(n * K), f(N * K), f(n * N), f(n * K), f(N * K), f(S * N)
        go, raw, o_ = f(S * N), f(S * N), f(S * N)
        ag, ap = i32(S * N), i32(S * N)
        pos_seg = (torch.arange(n, device=dev) // (n // S)).int()
        f64 = lambda numel: torch.full((numel,), SENTINEL, dtype=torch.float64, device=dev)
        gram, total, ptot = f64(int(lb.spt_fused_linear_pool_gram_len(K))), f64(2 * N + 1), f64(2 * K + 1)
        big = [torch.ones(max(256, N * K), device=dev) for _ in range(12)]
        outs += [h, gxs, gW, gm, o_, raw, ag, ap, gram, total, ptot]
        mode = precision.fused_mode()
        if entry == "fused_linear_bwd_pooled":
            each(["gout", "arg", "h", "xprev", "W", "gx"], lambda o: lb.spt_fused_linear_bwd_pooled_runs_f32(
                P(go) + o["gout"], P(ag) + o["arg"], P(perm), P(pos_seg), P(h) + o["h"], 1, r0, r1, rg, 1, N,
                P(big[0]), P(big[1]), P(big[2]), 0.01, P(big[3]), P(big[4]), P(big[5]), P(xs) + o["xprev"], K,
                P(big[6]), P(big[7]), P(big[8]), 0.01, P(W) + o["W"], P(gxs) + o["gx"], P(gW), P(ptot), -1, P(ws),
                ws.numel(), s))
        elif entry == "fused_linear_fwd_pool":
            assert lb.spt_fused_linear_pool_supported(K, N, mode)
            each(["x", "W", "out", "arg", "argpos", "raw"], lambda o: lb.spt_fused_linear_fwd_pool_runs_f32(
                P(xs) + o["x"], P(perm), P(pos_seg), P(rowptr), None, S, n, 1, r0, r1, rg, 1, K, P(W) + o["W"], N,
                P(big[0]), P(big[1]), P(big[2]), 1e-5, 0.01, P(big[3]), P(big[4]), P(big[5]), 0.01,
                P(o_) + o["out"], P(ag) + o["arg"], P(ap) + o["argpos"], P(raw) + o["raw"], P(gram), P(total),
                P(big[6]), P(big[7]), P(big[8]), P(big[9]), mode, P(ws), ws.numel(), s))
        else:
            assert lb.spt_fused_linear_pool_supported(K, N, mode)
            each(["gout", "raw", "argpos", "xprev", "W", "gx"], lambda o: lb.spt_fused_linear_bwd_pool_runs_f32(
                P(go) + o["gout"], P(raw) + o["raw"], P(ap) + o["argpos"], P(perm), P(pos_seg), None, S, 1, r0, r1, rg,
                1, N, P(big[0]), P(big[1]), P(big[2]), 0.01, P(big[3]), P(big[4]), P(big[5]), P(xs) + o["xprev"], K,
                P(big[6]), P(big[7]), P(big[8]), 0.01, P(W) + o["W"], P(gram), P(gm), P(gxs) + o["gx"], P(gW), P(ptot),
                mode, P(ws), ws.numel(), s))
    elif entry == "segcsr_max_affine_stream":
        # the row-streaming pool (c = 128 from 65 536 rows): f32 rows with the raw output, bf16 rows
        nn_, cc, SS = 65_536, 128, 16
        assert lb.spt_segcsr_max_affine_raw_supported(cc, nn_) and lb.spt_segcsr_max_affine_bf16_supported(cc, nn_)
        xb, ob, rb, ab = f(nn_ * cc), f(SS * cc), f(SS * cc), i32(SS * cc)
        pm = torch.arange(nn_, dtype=torch.int32, device=dev)
        rp = torch.arange(0, nn_ + 1, nn_ // SS, dtype=torch.int32, device=dev)
        outs += [ob, rb, ab]
        each(["x", "out", "arg", "raw"], lambda o: lb.spt_segcsr_max_affine_raw_f32(
            P(xb) + o["x"], 0, P(pm), P(rp), nn_, SS, cc, P(tab[0]), P(tab[1]), P(tab[2]), 0.01, None,
            P(ob) + o["out"], P(ab) + o["arg"], P(rb) + o["raw"], s))
        each(["x_bf16", "out", "arg"], lambda o: lb.spt_segcsr_max_affine_bf16(
            P(xb) + o["x_bf16"], P(pm), P(rp), nn_, SS, cc, P(tab[0]), P(tab[1]), P(tab[2]), 0.01, None,
            P(ob) + o["out"], P(ab) + o["arg"], s))
    elif entry in ("edge_attn_fwd", "edge_attn_bwd"):
        H, D, Dv, F = 16, 4, 4, 32
        e = n
        erow = torch.arange(n + 1, dtype=torch.int32, device=dev)
        tgt = torch.arange(n, dtype=torch.int32, device=dev)
        q, ea, o_, m, z = f(n * 192), f(e * F), f(n * 64), f(n * H), f(n * H)
        go, gq, gea = f(n * 64), f(n * 192), f(e * F)
        Wk, Wq, Wv = f(64 * F), f(64 * F), f(64 * F)
        outs += [o_, m, z, gq, gea]
        if entry == "edge_attn_fwd":
            each(["qkv", "edge_attr", "out", "Wk", "Wq", "Wv"], lambda o: lb.spt_edge_attn_fwd_ex_f32(
                P(q) + o["qkv"], n, H, D, Dv, P(erow), P(perm), P(tgt), e, P(ea) + o["edge_attr"], F,
                P(Wk) + o["Wk"], None, P(Wq) + o["Wq"], None, P(Wv) + o["Wv"], None, 0, 0.7, P(o_) + o["out"], P(m), P(z), -1, s))
        else:
            each(["qkv", "gqkv", "edge_attr", "gedge_attr", "out", "gout", "Wk", "Wq", "Wv"],
                 lambda o: lb.spt_edge_attn_bwd_ex_f32(
                P(q) + o["qkv"], n, H, D, Dv, P(erow), P(perm), P(tgt), None, None, None, None, e,
                P(ea) + o["edge_attr"], F, P(Wk) + o["Wk"], None, P(Wq) + o["Wq"], None, P(Wv) + o["Wv"], None, 0, 0.7, P(o_) + o["out"], P(m), P(z),
                P(go) + o["gout"], P(gq) + o["gqkv"], P(gea) + o["gedge_attr"], 0, None, None, None, None, None,
                None, -1, P(ws), ws.numel(), s))
    else:
        raise KeyError(entry)
