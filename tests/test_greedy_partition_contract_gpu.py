"""The entries of csrc/merge.hip under tests/guarded.py, called through the C ABI: every input
flush against its guard, every output cut to the byte between guards, the workspace exactly what
its query promises and NaN-filled (0xFF: -1 as an index, NaN as a float).  Asked for: intact
guards and the bits of the plain run through the Python wrappers.  Then the wrappers themselves
on exact, poisoned scratch, twice over, and on non-contiguous views."""
import numpy as np
import pytest
import torch

import greedy_partition_reference as R
from guarded import GuardedArena, exact_workspaces, poisoned_fresh_tensors

pytestmark = pytest.mark.gpu

REG = 2e-2


def arena_for(dev):
    return GuardedArena(dev, guard_byte=0xFF, fill_byte=0xFF)


def put(arena, t, label):
    return arena.place(t, guard_byte=0xFF if t.is_floating_point() else 0x00, label=label)


def fresh(arena, shape, dtype, label):
    n = int(np.prod(shape))
    return arena.take(n * torch.empty((), dtype=dtype).element_size(), dtype, tuple(shape), label)


def call(name, *args):
    from superpoint_transformer_amd import _lib
    dev = torch.cuda.current_device()
    st = getattr(_lib.lib, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args],
                                 _lib.stream_ptr(dev))
    _lib.check(st, name)


def query(name, *args):
    from superpoint_transformer_amd import _lib
    return getattr(_lib.lib, name)(*args)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def duplicated(n=40, e=900, seed=3):
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, n, size=(2, e)).astype(np.int64)
    ei[:, -560:] = np.array([[1], [0]])                             # a run longer than 512
    return n, ei, rng.uniform(0.5, 1.5, e).astype(np.float32)


@pytest.mark.parametrize("reduce", ["add", "mean", "min"])
@pytest.mark.parametrize("relabelled", [False, True])
def test_component_graph_between_guards(reduce, relabelled, dev):
    from superpoint_transformer_amd import partition as P
    n, ei, w = duplicated()
    index, C = None, n
    if relabelled:
        index, C = np.arange(n, dtype=np.int64) % 9, 9
    E = ei.shape[1]
    wantE, wantW = P.component_graph(_t(index, dev), _t(ei, dev), _t(w, dev), reduce, num_components=C)
    arena = arena_for(dev)
    g_ei, g_w = put(arena, _t(ei, dev), "edge_index"), put(arena, _t(w, dev), "edge_attr")
    g_idx = None if index is None else put(arena, _t(index, dev), "index")
    out_e = fresh(arena, (2, E), torch.int64, "out_edges")
    out_w = fresh(arena, (E,), torch.float32, "out_attr")
    counts = fresh(arena, (2,), torch.int64, "counts")
    nbytes = query("spt_component_graph_workspace_bytes", E)
    ws = arena.take(nbytes, label="ws")
    call("spt_component_graph_f32", g_ei, E, E, g_w, g_idx, n, C, P.REDUCES[reduce], out_e, E, out_w,
         counts, ws, nbytes)
    arena.check()
    k, bad = counts.tolist()
    assert bad == 0 and k == wantE.shape[1]
    assert torch.equal(out_e[:, :k], wantE) and torch.equal(out_w[:k].view(torch.int32),
                                                            wantW.view(torch.int32))
    tE, tW = R.component_graph(index, ei, w, reduce)
    assert np.array_equal(R.bits(wantE), tE) and np.array_equal(R.bits(wantW), R.bits(tW))


@pytest.mark.parametrize("case", ["grid", "trees"])
def test_round_entries_between_guards(case, dev):
    """One round, entry by entry, from the state the wrappers would hand over."""
    from superpoint_transformer_amd import partition as P
    K = P._Kernels
    if case == "grid":
        x, pos, ei = R.grid_case(24, 0.3, D=7, seed=2)
    else:
        x, pos, ei = R.grid_case(48, 0.0, D=2, seed=0)               # trees of 576 members
    C, D = x.shape
    sizes = np.random.default_rng(1).integers(1, 7, C).astype(np.int64)
    S = _t(sizes, dev)
    F = (_t(x, dev).double() * S.double()[:, None]).contiguous()
    Q = (_t(pos, dev).double() * S.double()[:, None]).contiguous()
    E, W = P.component_graph(None, _t(ei, dev), None, "add", num_components=C)
    ne = E.shape[1]
    # the plain run
    gain0 = torch.empty(ne, dtype=torch.float32, device=dev)
    best0 = K.choose(F, S, E, W, REG, gain=gain0)
    parent0, active0 = K.resolve(best0, S, 5, False)
    label0, new0 = K.relabel(parent0.clone())
    S0, F0, Q0 = K.accumulate(label0, new0, S, F, Q)
    tF, tS = F.cpu().numpy(), sizes
    tE, tW = R.component_graph(None, ei, None)
    assert np.array_equal(R.bits(gain0), R.bits(R.gains(tF, tS, tE, tW, REG)))

    arena = arena_for(dev)
    gF, gS, gQ = put(arena, F, "F"), put(arena, S, "S"), put(arena, Q, "Q")
    gE, gW = put(arena, E, "E"), put(arena, W, "W")
    mean = fresh(arena, (C, D), torch.float64, "mean")
    call("spt_merge_means_f64", gF, gS, C, D, mean)
    best = fresh(arena, (C,), torch.int64, "best")
    gain = fresh(arena, (ne,), torch.float32, "gain")
    call("spt_merge_choose_f64", mean, gS, C, D, gE, ne, ne, gW, REG, best, gain)
    parent = fresh(arena, (C,), torch.int64, "parent")
    active = fresh(arena, (1,), torch.int64, "active")
    call("spt_merge_resolve", best, gS, C, 5, 0, parent, active)
    hop = fresh(arena, (C,), torch.int64, "hop")
    changed = fresh(arena, (1,), torch.int64, "changed")
    call("spt_merge_jump", parent, C, hop, changed)
    arena.check()
    assert torch.equal(mean, F / S.double()[:, None])
    assert torch.equal(best, best0) and torch.equal(gain.view(torch.int32), gain0.view(torch.int32))
    assert torch.equal(parent, parent0) and int(active) == active0 > 0
    assert torch.equal(hop, parent0[parent0]) and int(changed) == int(not torch.equal(hop, parent0))

    g_label = put(arena, label0, "label")
    S2 = fresh(arena, (new0,), torch.int64, "S2")
    F2 = fresh(arena, (new0, D), torch.float64, "F2")
    Q2 = fresh(arena, (new0, 3), torch.float64, "Q2")
    nbytes = query("spt_merge_accumulate_workspace_bytes", C, new0)
    ws = arena.take(nbytes, label="ws")
    call("spt_merge_accumulate_f64", g_label, C, new0, gS, gF, D, gQ, S2, F2, Q2, ws, nbytes)
    arena.check()
    assert torch.equal(S2, S0)
    assert torch.equal(F2.view(torch.int64), F0.view(torch.int64))
    assert torch.equal(Q2.view(torch.int64), Q0.view(torch.int64))
    if case == "trees":
        assert int(torch.bincount(label0).max()) > R.LONG_RUN


def test_edge_weights_between_guards(dev):
    from superpoint_transformer_amd import partition as P
    x, pos, ei = R.grid_case(24, 0.3, D=7, seed=2)
    for rows in (pos, x, x[:, :1]):
        n, cols = rows.shape
        E = ei.shape[1]
        dist0, total0 = P.edge_lengths(_t(rows, dev), _t(ei, dev))
        arena = arena_for(dev)
        g_rows, g_ei = put(arena, _t(rows, dev), "rows"), put(arena, _t(ei, dev), "edge_index")
        dist = fresh(arena, (E,), torch.float32, "dist")
        total = fresh(arena, (1,), torch.float64, "sum")
        bad = fresh(arena, (1,), torch.int64, "bad")
        nbytes = query("spt_edge_weights_workspace_bytes", E)
        ws = arena.take(nbytes, label="ws")
        call("spt_edge_weights_f32", g_rows, n, cols, cols, g_ei, E, E, dist, total, bad, ws, nbytes)
        arena.check()
        assert int(bad) == 0 and float(total) == total0
        assert torch.equal(dist.view(torch.int32), dist0.view(torch.int32))
        assert np.array_equal(R.bits(dist), R.bits(R.edge_lengths(rows, ei)))


def _merge(dev, x, pos, ei, w, min_size, **kw):
    from superpoint_transformer_amd import partition as P
    S = torch.ones(x.shape[0], dtype=torch.int64, device=dev)
    return P.merge_components_by_contour_prior(_t(x, dev), S, _t(ei, dev), _t(w, dev), REG, min_size,
                                               P=_t(pos, dev), **kw)


def test_wrappers_on_exact_poisoned_memory(dev):
    """The Python surface with every ``_workspace`` request cut to the byte between guards and
    NaN-filled, and every fresh float tensor NaN-filled: still the twin's bits."""
    from superpoint_transformer_amd import transforms as T
    from superpoint_transformer_amd.data import Data
    n, dei, dw = duplicated()
    rng = np.random.default_rng(4)
    dx, dpos = rng.standard_normal((n, 4)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    gx, gpos, gei = R.grid_case(48, 0.0, D=2, seed=0)
    hx, hpos, hei = R.grid_case(24, 0.3, D=7, seed=2)
    arena = arena_for(dev)
    with poisoned_fresh_tensors(dev), exact_workspaces(arena):
        got_d = _merge(dev, dx, dpos, dei, dw, 4, reduce="mean")
        got_g = _merge(dev, gx, gpos, gei, None, 5)
        nag = T.GreedyContourPriorPartition(REG, [5, 30], edge_weight_mode="inverse_distance", d_0=1.5)(
            Data(x=_t(hx, dev), pos=_t(hpos, dev), edge_index=_t(hei, dev)))
    assert len(arena) > 0
    ones = lambda m: np.ones(m, dtype=np.int64)
    R.assert_same(got_d, R.merge(dx, ones(n), dei, dw, REG, 4, reduce="mean", P=dpos))
    R.assert_same(got_g, R.merge(gx, ones(len(gx)), gei, None, REG, 5, P=gpos))
    w = nag[0].edge_attr.cpu().numpy()                     # torch's elementwise kernels made them
    ref = R.weights_from_lengths(R.edge_lengths(hpos, hei), "inverse_distance", 1.5)
    assert (np.abs(w - ref) <= 2 * np.spacing(ref)).all()
    wI, _, (wX, wS, wE, _, wP) = R.merge_on_data(hx, hpos, hei, w, REG, 5)
    assert np.array_equal(R.bits(nag[0].super_index), wI)
    assert np.array_equal(R.bits(nag[1].x), R.bits(wX)) and np.array_equal(R.bits(nag[1].pos), R.bits(wP))
    assert np.array_equal(R.bits(nag[1].node_size), wS) and np.array_equal(R.bits(nag[1].edge_index), wE)


def test_two_runs_are_bitwise_equal(dev):
    x, pos, ei = R.grid_case(48, 0.3, D=7, seed=9)
    w = np.random.default_rng(9).uniform(0.5, 1.5, ei.shape[1]).astype(np.float32)
    a = _merge(dev, x, pos, ei, w, 30)
    b = _merge(dev, x, pos, ei, w, 30)
    assert a[1] == b[1] >= 3 and torch.equal(a[0], b[0])
    for s, t in zip(a[2], b[2]):
        assert np.array_equal(R.bits(s), R.bits(t))


def test_non_contiguous_views(dev):
    """Column slices, transposed and strided views go through the wrappers' normalisation."""
    from superpoint_transformer_amd import partition as P
    x, pos, ei = R.grid_case(24, 0.3, D=7, seed=2)
    N, E = x.shape[0], ei.shape[1]
    w = np.random.default_rng(2).uniform(0.5, 1.5, E).astype(np.float32)
    sizes = np.random.default_rng(3).integers(1, 4, N).astype(np.int64)
    plain = P.merge_components_by_contour_prior(_t(x, dev), _t(sizes, dev), _t(ei, dev), _t(w, dev), REG,
                                                30, P=_t(pos, dev))
    wide = torch.zeros((N, 12), device=dev)
    wide[:, 2:9], wide[:, 9:] = _t(x, dev), _t(pos, dev)
    ei_t = _t(np.ascontiguousarray(ei.T), dev).t()                   # [2, E] with strides (1, 2)
    w2 = torch.zeros(2 * E, device=dev)
    w2[::2] = _t(w, dev)
    s2 = torch.zeros((N, 2), dtype=torch.int64, device=dev)
    s2[:, 1] = _t(sizes, dev)
    assert not ei_t.is_contiguous() and not wide[:, 2:9].is_contiguous()
    views = P.merge_components_by_contour_prior(wide[:, 2:9], s2[:, 1], ei_t, w2[::2], REG, 30,
                                                P=wide[:, 9:])
    assert plain[1] == views[1] and torch.equal(plain[0], views[0])
    for s, t in zip(plain[2], views[2]):
        assert np.array_equal(R.bits(s), R.bits(t))
    R.assert_same(views, R.merge(x, sizes, ei, w, REG, 30, P=pos))
    d0, t0 = P.edge_lengths(_t(pos, dev), _t(ei, dev))
    d1, t1 = P.edge_lengths(wide[:, 9:], ei_t)
    assert torch.equal(d0, d1) and t0 == t1
    gE, gW = P.component_graph(s2[:, 1] % 5, ei_t, w2[::2], "max", num_components=5)
    hE, hW = P.component_graph(_t(sizes % 5, dev), _t(ei, dev), _t(w, dev), "max", num_components=5)
    assert torch.equal(gE, hE) and torch.equal(gW, hW)
