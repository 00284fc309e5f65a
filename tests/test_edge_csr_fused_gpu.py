"""The edge view of an attention graph through the one entry ``spt_edge_csr_build`` (stable sort
of (source, edge, target) triples whose last pass writes the tables, the mirror check riding on the
first read) against the route it replaces (pair sort + one kernel per table), switched by
``csr.use_fused_edge_build``.  Every output is an integer array and a stable sort has exactly one
result, so every comparison here is ``torch.equal``: erowptr, eperm, tgt_sorted, src_sorted(), the
64-int tile records, the inverse of eperm and the verdict word of the mirror check."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TARGET = 1 << 6          # mode word: tile records in target order (64 ints)


def _declare(ei, m):
    if m is not None:
        ei._spt_mirror_pairs = int(m)
    return ei


def _layout(lo, hi, loops, dev, declare=True):
    """[i<j | j>i | loops] from the (lo, hi) pairs and the loop nodes."""
    lo, hi, loops = (torch.as_tensor(t, dtype=torch.long) for t in (lo, hi, loops))
    ei = torch.stack([torch.cat([lo, hi, loops]), torch.cat([hi, lo, loops])]).to(dev)
    return _declare(ei, lo.numel() if declare else None)


def _random(seed, n, m, loops, dev, lo_node=0, hi_node=None, declare=True):
    gen = torch.Generator().manual_seed(seed)
    hi_node = n if hi_node is None else hi_node
    a = torch.randint(lo_node, hi_node, (m,), generator=gen)
    b = torch.randint(lo_node, hi_node, (m,), generator=gen)
    keep = a != b
    return _layout(torch.minimum(a, b)[keep], torch.maximum(a, b)[keep], loops, dev, declare)


def _tables(ei, n, fused):
    """Build the view of ``ei`` with the switch at ``fused``; the six tables + the verdict word.
    A failed structure check is returned as its message instead of being raised."""
    from superpoint_transformer_amd import csr
    m = getattr(ei, csr.MIRROR_ATTR, None)
    old = csr.use_fused_edge_build(fused)
    try:
        csr.forget(ei)
        ec = csr.edge_csr_of(ei, n)
        out = {"erowptr": ec.erowptr, "eperm": ec.eperm, "tgt_sorted": ec.tgt_sorted,
               "src_sorted": ec.src_sorted(), "tile_ids": ec.tile_ids(TARGET)}
        out["inv"] = ec._inv
        out["flag"] = None if ec._flag is None else ec._flag.clone()
        try:
            csr.verify_adopted(block=True)
            out["error"] = None
        except csr.StaleCSRError as err:
            out["error"] = str(err)
            _declare(ei, m)                  # (the failed hint was taken off the tensor)
        torch.cuda.synchronize()
        return out
    finally:
        csr.use_fused_edge_build(old)
        csr.forget(ei)


def _same(a, b, what):
    for k in a:
        if torch.is_tensor(a[k]) or torch.is_tensor(b[k]):
            assert torch.is_tensor(a[k]) and torch.is_tensor(b[k]), f"{what}: {k} missing on one side"
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, f"{what}: {k} shape / dtype"
            assert torch.equal(a[k], b[k]), f"{what}: {k} differs"
        else:
            assert a[k] == b[k], f"{what}: {k}: {a[k]!r} != {b[k]!r}"


def _check(ei, n, what, expect_error=False):
    ref = _tables(ei, n, False)
    got = _tables(ei, n, True)
    _same(ref, got, what)
    order = torch.sort(ei[0], stable=True).indices
    assert torch.equal(got["eperm"].long(), order), f"{what}: eperm is not the stable argsort"
    assert (got["error"] is not None) == expect_error
    return ref


@pytest.mark.parametrize("e,pairs,loops", [(1, 0, 1), (15, 5, 5), (16, 6, 4), (17, 6, 5), (33, 12, 9)])
def test_tile_tail(e, pairs, loops, dev):
    """E around one and two tiles of 16 edges: the tail of the last record repeats the last edge."""
    n = max(loops, 7)
    ei = _random(e, n, 4 * pairs + 8, list(range(loops)), dev)
    M = ei._spt_mirror_pairs
    keep = torch.cat([torch.arange(pairs), M + torch.arange(pairs), 2 * M + torch.arange(loops)]).to(dev)
    ei = _declare(ei[:, keep].contiguous(), pairs)
    assert ei.shape[1] == e
    _check(ei, n, f"E = {e}")


@pytest.mark.parametrize("n", [1, 2, 256, 257, 2049, (1 << 16) + 1, (1 << 22) + 1])
def test_digit_and_pass_boundaries(n, dev):
    """1, 8, 9, 12, 17 and 23 key bits: one pass of the narrowest and of the widest digit, the first
    two-pass size (5 + 4 bits), 6 + 6, the first three-pass size, and a graph past 2^22 nodes
    (8 + 8 + 7: both scratch triples and the tables)."""
    gen = torch.Generator().manual_seed(n)
    if n == 1:
        ei = _layout([], [], [0] * 3000, dev)
    else:
        loops = torch.randint(0, n, (500,), generator=gen)
        ei = _random(n, n, 1500, loops, dev)
    _check(ei, n, f"N = {n}")


def test_nodes_without_edges(dev):
    """No edge at the front, in the middle and at the end of the node range: runs of equal row
    pointers (the long-run path of the boundary kernel among them)."""
    n = 3000
    a = _random(1, n, 900, list(range(100, 1200, 7)), dev, 100, 1200)
    b = _random(2, n, 900, list(range(1800, 2900, 5)), dev, 1800, 2900)
    Ma, Mb = a._spt_mirror_pairs, b._spt_mirror_pairs
    parts = [a[:, :Ma], b[:, :Mb], a[:, Ma:2 * Ma], b[:, Mb:2 * Mb], a[:, 2 * Ma:], b[:, 2 * Mb:]]
    ei = _declare(torch.cat(parts, 1).contiguous(), Ma + Mb)
    ref = _check(ei, n, "empty nodes")
    rp = ref["erowptr"]
    assert int(rp[100]) == 0 and int(rp[1200]) == int(rp[1800]) and int(rp[2900]) == int(rp[n]) == ei.shape[1]


def test_loops_only_no_loops_and_duplicates(dev):
    n = 777
    _check(_layout([], [], list(range(n)), dev), n, "loops only")
    _check(_random(3, n, 4000, [], dev), n, "no loops")
    lo = torch.tensor([3, 3, 3, 10, 10, 500] * 200)
    hi = torch.tensor([9, 9, 9, 700, 700, 776] * 200)
    _check(_layout(lo, hi, [5, 5, 5, 776], dev), n, "duplicate pairs")


def test_one_node_owns_every_edge(dev):
    """One digit receives all the elements, in every pass: a list of loops at one node (declared),
    and a star of 5000 edges out of node 41 (no mirror structure, no hint: the sort and the table
    pass still run, the records come from the sorted target view on both sides)."""
    _check(_layout([], [], [7] * 5000, dev), 300, "loops at one node")
    gen = torch.Generator().manual_seed(4)
    star = torch.stack([torch.full((5000,), 41), torch.randint(0, 300, (5000,), generator=gen)]).to(dev)
    ref = _check(star, 300, "star, no hint")
    assert ref["inv"] is None and ref["flag"] is None


def test_several_workgroups(dev):
    """E = 70 001 on 4 099 nodes: 18 sort tiles, 13 bits (two passes of 7 + 6)."""
    ei = _random(5, 4099, 32951, list(range(4099)), dev)
    M = ei._spt_mirror_pairs
    pad = 32951 - M                                   # pairs dropped as a == b: repeat the first ones
    idx = torch.cat([torch.arange(M), torch.arange(pad)]).to(dev)
    ei = _declare(torch.cat([ei[:, :M][:, idx], ei[:, M:2 * M][:, idx], ei[:, 2 * M:]], 1).contiguous(), 32951)
    assert ei.shape[1] == 70001
    _check(ei, 4099, "70 001 edges")


def test_four_cloud_batch(dev):
    """A batch of four clouds as the train-batch scene builds it: every third of the layout is
    sorted by cloud, no edge crosses two clouds."""
    from superpoint_transformer_amd.synthetic import _edges
    gen = torch.Generator().manual_seed(6)
    cloud = torch.repeat_interleave(torch.arange(4), torch.tensor([700, 300, 900, 500]))
    ei = _edges(gen, 2400, 14000, "cpu", cloud=cloud)
    _check(_declare(ei.to(dev), ei._spt_mirror_pairs), 2400, "four clouds")


def test_wrong_hints_raise_with_the_same_bits(dev):
    """A wrong M, a broken pair and a false loop: the same verdict word and the same StaleCSRError."""
    n = 900
    good = _random(7, n, 3600, list(range(n)), dev)
    M = good._spt_mirror_pairs

    def edited(fn, m=M):
        ei = good.clone()
        fn(ei)
        return _declare(ei.clone(), m)

    cases = {"wrong M": (edited(lambda ei: None, M - 1), 3),
             "broken pair": (edited(lambda ei: ei[1].__setitem__(M + 5, (ei[1, M + 5] + 1) % n)), 1),
             "false loop": (edited(lambda ei: ei[1].__setitem__(2 * M + 9, (ei[1, 2 * M + 9] + 1) % n)), 2)}
    for what, (ei, bits) in cases.items():
        ref = _check(ei, n, what, expect_error=True)
        assert int(ref["flag"]) == bits, what
        assert "mirror" in ref["error"]


def test_build_under_capture_and_twice(dev):
    """Two eager builds of one input are equal; the build captured in a graph and replayed twice
    gives those tables both times (the scratch is written before it is read in every replay)."""
    from superpoint_transformer_amd import csr
    n = 2049
    ei = _random(8, n, 6000, list(range(0, n, 2)), dev)
    first = _tables(ei, n, True)
    _same(first, _tables(ei, n, True), "second eager build")
    assert csr.use_fused_edge_build(True) is True
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        csr.forget(ei)
        csr.edge_csr_of(ei, n)
        csr.forget(ei)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ec = csr.edge_csr_of(ei, n)
    names = ("erowptr", "eperm", "tgt_sorted", "inv", "tile_ids", "flag")
    held = {"erowptr": ec.erowptr, "eperm": ec.eperm, "tgt_sorted": ec.tgt_sorted, "inv": ec._inv,
            "tile_ids": ec.tile_ids(TARGET), "flag": ec._flag, "src_sorted": ec.src_sorted()}
    for rep in range(2):
        for t in held.values():
            t.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        for k in names + ("src_sorted",):
            assert torch.equal(held[k], first[k]), f"replay {rep}: {k}"
    csr.verify_adopted(block=True)
    csr.forget(ei)


def test_attention_is_bitwise_the_same(dev):
    """One attention forward + backward on a 300-node graph with the switch off and on.  In the
    source order the backward is reproducible bit for bit, so everything is compared bitwise
    there; in the default target order dk / dv are float atomics whose order changes from run to
    run with either route, so only the forward (no atomics) is held to the bit."""
    from superpoint_transformer_amd import csr, nn as N, precision
    n = 300
    ei = _random(9, n, 1200, list(range(n)), dev)
    gen = torch.Generator().manual_seed(10)
    blk = N.SelfAttentionBlock(64, num_heads=16, out_dim=None, qk_dim=4, in_rpe_dim=32,
                               k_rpe=True, q_rpe=True, v_rpe=True).to(dev)
    x = torch.randn(n, 64, generator=gen).to(dev)
    ea = (torch.randn(ei.shape[1], 32, generator=gen) * 0.5).to(dev)
    gw = torch.randn(n, 64, generator=gen).to(dev)

    def run(fused):
        old = csr.use_fused_edge_build(fused)
        try:
            csr.forget(ei)
            xd, ead = x.clone().requires_grad_(), ea.clone().requires_grad_()
            blk.zero_grad(set_to_none=True)
            out = blk(xd, ei, edge_attr=ead)
            (out * gw).sum().backward()
            torch.cuda.synchronize()
            csr.verify_adopted(block=True)
            return {"out": out.detach(), "g_x": xd.grad, "g_edge_attr": ead.grad,
                    **{"g_" + k: p.grad.clone() for k, p in blk.named_parameters()}}
        finally:
            csr.use_fused_edge_build(old)
            csr.forget(ei)

    with precision.attention_backward_order("source"):
        _same(run(False), run(True), "source order")
    off, on = run(False), run(True)
    assert torch.equal(off["out"], on["out"])
    for k in off:
        # (f32 sums of a few thousand terms in another order: ~1e-7 * sqrt(terms) of the largest value)
        assert float((off[k] - on[k]).abs().max()) <= 1e-4 * float(off[k].abs().max()), k
