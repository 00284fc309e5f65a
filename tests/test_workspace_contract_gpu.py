"""Every ``spt_*_workspace_bytes`` promise, kept to the byte.

The Python side hands every entry point one grow-only scratch buffer (``ops._workspace``: at least
1 MiB, rounded up by the caching allocator, as large as the largest earlier request), so no other
test runs a kernel against a workspace of exactly the size its size function returned: a write
past the plan lands in slack.  Here each entry point runs with the workspace - and, where the
caller computes their length, the outputs - cut to the byte out of a guarded arena
(tests/guarded.py: 1 MiB of a fixed byte on both sides).  Three assertions per call:

  1. the guards are intact (``arena.check()``);
  2. the result is right: same reference and same bar as the entry point's own test (named at
     each test below); integer outputs bit-exact;
  3. the result is bit-identical to the same call through the normal grow-only ``_workspace``.

Every call then runs a third time on an arena whose guards AND contents are 0xFF (NaN in every
float format, -1 as an integer), through the wrappers with ``torch.empty`` and its kin handing
out NaN as well: a workgroup that skips its partial table, a scan that leaves a partial
unwritten or an output element no kernel wrote is then read as NaN instead of as what the last
call of the same shape left there.  Two more assertions: these guards are intact too, and the
result is bit-identical to the generous run.

Scan lengths stay below 2^21: even a partials region with no room at all would then overflow by
2 KiB at most, far inside a guard.

Shapes and the plan boundary each one probes (SCAN_TILE = SORT_TILE = 4096; regions are aligned
to 256 B = 64 u32 entries; L = length of the scanned array):

size function                          shapes                                 boundary probed
-------------------------------------  -------------------------------------  ------------------------------------------
spt_relabel_consecutive_~              n_range + 1 = L in SCAN_L              L = 4095 | 4096 | 4097: one / two scan tiles;
spt_radius_ball_~                      n + 1 = L in SCAN_L                      262 144 | 262 145: 64 partials fill the 256-B
spt_neighbors_dense_to_csr_~           n + 1 = L in SCAN_L                      region / the 65th opens a second one;
spt_select_edges_~                     E + 1 = L in SCAN_L                      1 048 577: 257 partials, the carry loop of
spt_adjacency_count_~                  n + 1 = L in SCAN_L                      scan_partials_kernel (> 256 chunks)
spt_csr_build_~                        n in 4095, 4096, 4097, 12 305 x        n: one / two / four sort tiles (histogram rows);
                                       num_seg in 256, 257, 65 536, 65 537,   num_seg: 8|9, 16|17, 24|25 key bits = 1|2, 2|3,
                                       2^24 + 1                               3|4 radix passes
spt_cluster_graph_edges_~              S = 8738, 8739 with k_max = 30         m + 1 = 262 141 | 262 171: the flag scan needs
                                                                              64 | 65 partials (the sort's own region holds 64)
spt_sparse_sample_~                    n = 300 000, num_seg = 262 144,        num_seg + 1 = 262 145: 65 partials (the sort's
                                       with and without a mask                region, sized from n, holds 64)
spt_cluster_select_~                   fixture (k = 40) and k + 1 = 4097,     one / two scan tiles for the sizes scan, two /
                                       n_sub + 1 = 9001                       three for the presence scan
spt_grid_knn_~                         11 003 points, K = 46: grid chosen by  ncells + 1 row pointers, three sort tiles of
                                       the probes and cell 0.11               points; cell 0.11: ~1.5e8 cells, 28 key bits
                                                                              (4 radix passes: the grid regime)
spt_grid_count_cells_~                 300 000 points, cell 0.5 and 0.07      bitmap of ncells / 32 words: 3 | 900 regions
spt_spatial_order_~                    n = 4096, 4097 x cell 1.0, 0.05        one | two sort tiles; 10 | 23 key bits
spt_unit_sphere_~                      (6144, 3), (6147, 3), (5000, 37)       average segment 2048 | 2049 rows: 1 | 2 slices
spt_graphnorm_~                        (5000, 32, B 3), (60 000, 128, B 40)   below / at the 128-block floor; one / two graph
                                                                              windows of the LDS table
spt_graphnorm_bwd_stats_sparse_~       pool cases below (S 900 B 3, S 800)    1024 * B * (2 d + 1) doubles: B = 3 | 1
spt_fused_linear_~                     pool cases below: 12->32->64(->128)    one table per (K, N): 12x32, 32x64, 64x128
spt_fused_linear_pool_~                (64, 128) rows 40 001 B 3;             the two built top layers
                                       (32, 64) rows 25 000 B 1
spt_edge_attn_bwd_~                    n 100, no edge features (H 8, D 8)     weight-gradient tables only
spt_edge_attn_bwd_ex_~                 n 300 e ~3300; n 4000 e ~2750          e > 0.93 n | e < 0.93 n: the edge-lane layout /
                                                                              the target-order layout is the larger one
spt_skinny_dw_~                        (64, 192) rows 4099, 70 001            65 | 256 = DW_BLOCKS workgroups of partials
spt_narrow_linear_bwd_~                (64, 13) rows 4099, 70 001             65 | 256 = NARROW_BLOCKS workgroups
spt_cross_entropy_~ (both losses)      rows 256, 257, 70 001, C = 13          one | two CE_BLOCK rows of f64 partials
spt_ground_bounds_~                    n = 100 003, 131 041, 262 145          391 | 512 | 1024 = the cap of reduce blocks
spt_ground_trim_~                      same clouds                            words + 1 = 3127 | 4097 | 8193: 1 | 2 | 3 tiles
spt_ground_ransac_~                    fixture 'both', 64 drawn triplets      fixed plan (MAX_H planes + 512 moment rows)
spt_point_color_~                      n = 257, 100 003 (u8 and f32)          fixed 256 B flag word
spt_adjacency_stats_~                  n = 256, 257, 100 003 (K 45, k 10)     1 | 2 | 391 workgroups of f64 partials
spt_adjacency_fill_~                   same tables                            cursor / staging rows of n and E entries
"""
import ctypes
import math
import zlib

import numpy as np
import pytest
import torch

from guarded import GuardedArena, exact_workspaces, poisoned_fresh_tensors
from oracle import spt_oracle as O

pytestmark = pytest.mark.gpu

SCAN_L = [4095, 4096, 4097, 262_144, 262_145, 1_048_577]
assert max(SCAN_L) < 1 << 21


# ---- plumbing -------------------------------------------------------------------------------------
def lib():
    from superpoint_transformer_amd import _lib
    return _lib


def flat(x):
    """Tensors of a nested result, in a fixed order."""
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
        assert s.shape == t.shape and s.dtype == t.dtype, (what, i, s.shape, t.shape)
        s8 = s.detach().contiguous().reshape(-1).view(torch.uint8)
        t8 = t.detach().contiguous().reshape(-1).view(torch.uint8)
        assert torch.equal(s8, t8.to(s8.device)), f"{what}: output {i} differs between the exact and the generous workspace"


class Generous:
    """The normal path: the grow-only buffer with its real (larger) size, plain outputs."""

    def __init__(self, dev):
        self.dev = dev

    def ws(self, nbytes):
        from superpoint_transformer_amd.ops import _workspace
        t = _workspace(nbytes, self.dev)
        assert t.numel() >= max(nbytes, 1 << 20)
        return t, t.numel()

    def out(self, dtype, *shape, label=None):
        return torch.empty(shape, dtype=dtype, device=self.dev)


class Exact:
    """Workspace and outputs cut to the byte out of a guarded arena."""

    def __init__(self, dev):
        self.dev = dev
        self.arena = GuardedArena(dev)

    def ws(self, nbytes):
        return self.arena.take(nbytes, label="ws"), nbytes

    def out(self, dtype, *shape, label=None):
        nbytes = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
        return self.arena.take(nbytes, dtype, shape, label=label)


class Poisoned(Exact):
    """Exact, with NaN in every byte the call may read without having written it: the guards and
    the contents of the workspace and of the outputs are 0xFF (NaN as a float, -1 as an integer)."""

    def __init__(self, dev):
        self.dev = dev
        self.arena = GuardedArena(dev, guard_byte=0xFF, fill_byte=0xFF)


def c_call(dev, call, what):
    """``call(alloc)`` through the C ABI with the generous, the exact and the poisoned allocator:
    guards intact, same bits; returns the exact run's result."""
    with torch.cuda.device(dev):
        gen = call(Generous(dev))
        ex_alloc = Exact(dev)
        ex = call(ex_alloc)
        po_alloc = Poisoned(dev)
        po = call(po_alloc)
    ex_alloc.arena.check()
    same_bits(gen, ex, what)
    po_alloc.arena.check()
    same_bits(gen, po, what + " (poisoned scratch and outputs)")
    return ex


def wrapped(dev, fn, what, sizes=(), any_of=(), bits_of=None):
    """``fn()`` through the Python wrappers with the normal ``_workspace``, with the arena in its
    place, and with a NaN-filled arena while every fresh floating tensor is NaN-filled too (a
    partial table, an output or an intermediate read without having been written in the same
    call then changes the result); ``sizes``: byte counts that must have been asked of the arena (the entry point ran,
    with exactly what its size function returned); ``any_of``: at least one of these was;
    ``bits_of``: the part of the result compared bit for bit (default: all of it)."""
    gen = fn()
    arena = GuardedArena(dev)
    with exact_workspaces(arena):
        ex = fn()
    asked = arena.sizes()
    assert asked, f"{what}: no workspace was asked for"
    for nb in sizes:
        assert int(nb) in asked, f"{what}: no request of {nb} bytes among {sorted(set(asked))}"
    assert not any_of or any(int(nb) in asked for nb in any_of), (what, any_of, sorted(set(asked)))
    pick = bits_of or (lambda r: r)
    same_bits(pick(gen), pick(ex), what)
    poisoned = GuardedArena(dev, guard_byte=0xFF, fill_byte=0xFF)
    with poisoned_fresh_tensors(dev):
        with exact_workspaces(poisoned):              # checks its guards on the way out
            po = fn()
    assert poisoned.sizes() == asked, f"{what}: the poisoned run asked for other workspaces"
    same_bits(pick(gen), pick(po), what + " (poisoned scratch and fresh tensors)")
    return ex


def ok(st, name):
    lib().check(st, name)


def P(t):
    return lib().ptr(t)


def stream(dev):
    return lib().stream_ptr(dev)


def seeded(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ---- scans: L = 4095 .. 1 048 577 -------------------------------------------------------------------
@pytest.mark.parametrize("L", SCAN_L)
def test_relabel_consecutive(L, dev):
    """Reference and bar: tests/test_select_gpu.py::test_consecutive_cluster_matches_the_oracle
    (O.consecutive_cluster = torch.unique, bit-exact)."""
    from superpoint_transformer_amd.data import consecutive_cluster
    n_range = k = L - 1
    src = torch.randint(0, n_range, (k,), generator=seeded("relabel", L))
    src[0], src[1] = n_range - 1, 0                       # both ends of the range are present
    rinv, rperm = O.consecutive_cluster(src)
    d = src.to(dev)
    lb = lib().lib

    def call(A):
        ws, wsb = A.ws(lb.spt_relabel_consecutive_workspace_bytes(n_range))
        inv = A.out(torch.int64, k, label="new_values")
        uniq = A.out(torch.int64, min(k, n_range), label="uniques")
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        ok(lb.spt_relabel_consecutive(P(d), None, k, n_range, P(inv), P(uniq), P(count), P(ws), wsb,
                                      stream(dev)), "spt_relabel_consecutive")
        return inv, uniq[:int(count)]

    inv, uniq = c_call(dev, call, f"relabel_consecutive L={L}")
    assert torch.equal(inv.cpu(), rinv) and torch.equal(uniq.cpu(), src[rperm])
    w = wrapped(dev, lambda: consecutive_cluster(d, n_range), "consecutive_cluster",
                [lb.spt_relabel_consecutive_workspace_bytes(n_range)])
    same_bits(w, (inv, uniq), "wrapper against the C ABI")


@pytest.mark.parametrize("L", SCAN_L)
def test_radius_ball(L, dev):
    """Reference: the kernel's own f32 expression sqrt(dx*dx + dy*dy + dz*dz) <= r evaluated by
    torch on the CPU (IEEE f32, no contraction on either side), bit-exact indices - the rule
    tests/test_batch_pipeline_gpu.py::test_radius_subgraphs_match_the_brute_force_neighbourhoods
    checks through the transform."""
    n = L - 1
    g = seeded("ball", L)
    pos = (torch.rand(n, 3, generator=g) * 10).float()
    batch = torch.randint(0, 2, (n,), generator=g)
    c, r = (5.0, 4.5, 5.25), 4.0
    lb = lib().lib
    dpos, dbatch = pos.to(dev), batch.to(dev)
    center = (ctypes.c_float * 3)(*c)
    for cyl, use_batch in ((0, False), (1, True)):
        dx, dy = pos[:, 0] - c[0], pos[:, 1] - c[1]
        dz = (pos[:, 2] - c[2]) * (0.0 if cyl else 1.0)
        keep = (dx * dx + dy * dy + dz * dz).sqrt() <= r
        if use_batch:
            keep &= batch == 1
        ref = torch.nonzero(keep).view(-1)

        def call(A):
            ws, wsb = A.ws(lb.spt_radius_ball_workspace_bytes(n))
            out = A.out(torch.int64, n, label="out_idx")
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            ok(lb.spt_radius_ball_f32(P(dpos), n, ctypes.cast(center, ctypes.c_void_p), r, cyl,
                                      P(dbatch) if use_batch else None, 1, P(out), P(count), P(ws),
                                      wsb, stream(dev)), "spt_radius_ball_f32")
            return out[:int(count)]

        got = c_call(dev, call, f"radius_ball L={L} cyl={cyl}")
        assert 0 < ref.numel() < n and torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("L", SCAN_L)
def test_neighbors_dense_to_csr(L, dev):
    """Reference and bar: tests/test_neighbors_gpu.py::
    test_neighbors_dense_to_csr_kernel_matches_reference_rule (O.neighbors_dense_to_csr, bit-exact)."""
    from superpoint_transformer_amd.neighbors import neighbors_dense_to_csr
    n, k = L - 1, 3
    g = seeded("dense", L)
    nn = torch.randint(0, 1000, (n, k), generator=g)
    nn[torch.rand(n, k, generator=g) < 0.4] = -1
    nn[-1] = torch.tensor([7, -1, 9])                       # the last row is not empty
    rp, rv, rs = O.neighbors_dense_to_csr(nn)
    d = nn.to(dev)
    lb = lib().lib

    def call(A):
        ws, wsb = A.ws(lb.spt_neighbors_dense_to_csr_workspace_bytes(n))
        ptr = A.out(torch.int64, n + 1, label="ptr")
        val = A.out(torch.int64, n * k, label="val")
        sizes = A.out(torch.int64, n, label="sizes")
        ok(lb.spt_neighbors_dense_to_csr(P(d), n, k, P(ptr), P(val), P(sizes), P(ws), wsb, stream(dev)),
           "spt_neighbors_dense_to_csr")
        return ptr, val[:int(ptr[-1])], sizes

    ptr, val, sizes = c_call(dev, call, f"neighbors_dense_to_csr L={L}")
    assert torch.equal(ptr.cpu(), rp) and torch.equal(val.cpu(), rv) and torch.equal(sizes.cpu(), rs)
    w = wrapped(dev, lambda: neighbors_dense_to_csr(d), "neighbors_dense_to_csr",
                [lb.spt_neighbors_dense_to_csr_workspace_bytes(n)])
    same_bits(w, (ptr, val, sizes), "wrapper against the C ABI")


@pytest.mark.parametrize("L", SCAN_L)
def test_select_edges(L, dev):
    """Reference and bar: the mask expression of tests/test_select_gpu.py::test_select_at_scene_scale
    (both ends kept, relabelled, in order; bit-exact)."""
    E, n = L - 1, 5000
    g = seeded("edges", L)
    e = torch.randint(0, n, (2, E), generator=g)
    idx = torch.randperm(n, generator=g)[:3000]
    inv_ref = torch.full((n,), -1, dtype=torch.long)
    inv_ref[idx] = torch.arange(idx.numel())
    keep = (inv_ref[e[0]] >= 0) & (inv_ref[e[1]] >= 0)
    keep_ref = torch.nonzero(keep).view(-1)
    de, didx = e.to(dev).contiguous(), idx.to(dev)
    lb = lib().lib
    inv = torch.empty(n, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        ok(lb.spt_index_inverse(P(didx), idx.numel(), n, P(inv), stream(dev)), "spt_index_inverse")
    assert torch.equal(inv.cpu(), inv_ref)

    def call(A):
        ws, wsb = A.ws(lb.spt_select_edges_workspace_bytes(E))
        out_e = A.out(torch.int64, 2, E, label="out_edges")
        idx_e = A.out(torch.int64, E, label="idx_edge")
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        ok(lb.spt_select_edges(P(de), E, E, P(inv), n, P(out_e), E, P(idx_e), P(count), P(ws), wsb,
                               stream(dev)), "spt_select_edges")
        kept = int(count)
        return out_e[:, :kept], idx_e[:kept]

    out_e, idx_e = c_call(dev, call, f"select_edges L={L}")
    assert torch.equal(idx_e.cpu(), keep_ref) and torch.equal(out_e.cpu(), inv_ref[e[:, keep]])


@pytest.mark.parametrize("L", SCAN_L)
def test_adjacency_count(L, dev):
    """Row i lists i + 1 and (two rows of three) i + 7 on a ring: no pair is mutual, so every valid
    entry survives and belongs to the row of its smaller end.  Reference: torch.bincount +
    torch.cumsum, bit-exact (the rule tests/test_adjacency_gpu.py checks through the graph)."""
    n, k = L - 1, 2
    i = torch.arange(n)
    nn = torch.stack([(i + 1) % n, (i + 7) % n], 1)
    nn[i % 3 == 0, 1] = -1
    valid = nn >= 0
    lo = torch.minimum(i.view(-1, 1).expand(n, k), nn)[valid]
    counts = torch.bincount(lo, minlength=n)
    ref_start = torch.cat((torch.zeros(1, dtype=torch.long), counts.cumsum(0)))
    ref_keep = valid.long() @ torch.tensor([1, 2])
    d = nn.to(dev).contiguous()
    linked = torch.ones(n, dtype=torch.uint8, device=dev)
    lb = lib().lib

    def call(A):
        ws, wsb = A.ws(lb.spt_adjacency_count_workspace_bytes(n))
        keep = A.out(torch.int64, n, label="keep")
        row_start = A.out(torch.int32, n + 1, label="row_start")
        ok(lb.spt_adjacency_count(P(d), n, k, k, P(linked), None, None, 0, 0, P(keep), P(row_start),
                                  P(ws), wsb, stream(dev)), "spt_adjacency_count")
        return keep, row_start

    keep, row_start = c_call(dev, call, f"adjacency_count L={L}")
    assert torch.equal(keep.cpu(), ref_keep)
    assert torch.equal(row_start.cpu().long(), ref_start)


# ---- CSR build / radix sort ---------------------------------------------------------------------------
@pytest.mark.parametrize("num_seg", [256, 257, 65_536, 65_537, (1 << 24) + 1])
@pytest.mark.parametrize("n", [4095, 4096, 4097, 3 * 4096 + 17])
def test_csr_build(n, num_seg, dev):
    """Reference: O.csr_view (torch.sort(stable=True) + bincount / cumsum), bit-exact, as in
    tests/test_segcsr_gpu.py.  The generous side is csr.build_csr (its own torch.empty scratch)."""
    from superpoint_transformer_amd.csr import build_csr
    idx = torch.randint(0, num_seg, (n,), generator=seeded("csr", n, num_seg))
    idx[0], idx[1], idx[2] = num_seg - 1, 0, num_seg - 1      # every key bit is used
    rperm, rrow = O.csr_view(idx, num_seg)
    d = idx.to(dev)
    lb = lib().lib
    nbytes = lb.spt_csr_build_workspace_bytes(n, num_seg)
    gen = build_csr(d, num_seg)
    for A in (Exact(dev), Poisoned(dev)):
        ws, wsb = A.ws(nbytes)
        perm = A.out(torch.int32, n, label="perm")
        rowptr = A.out(torch.int32, num_seg + 1, label="rowptr")
        with torch.cuda.device(dev):
            ok(lb.spt_csr_build(P(d), n, num_seg, P(perm), P(rowptr), P(ws), wsb, stream(dev)), "spt_csr_build")
        A.arena.check()
        assert torch.equal(perm.cpu(), rperm)
        assert torch.equal(rowptr, rrow.to(dev))
        same_bits((gen.perm, gen.rowptr), (perm, rowptr), f"csr_build n={n} num_seg={num_seg} {type(A).__name__}")


# ---- cluster graph: S * k_max just under and just over 262 143 ---------------------------------------
_CLUSTERS = {}


def clusters(S):
    """S clusters of about 8 points and the oracle's graph, computed once (about 4 s on the CPU)."""
    if S not in _CLUSTERS:
        g = seeded("clusters", S)
        sizes = torch.randint(1, 16, (S,), generator=g)
        idx = torch.repeat_interleave(torch.arange(S), sizes)
        idx = idx[torch.randperm(idx.numel(), generator=g)]
        centre = torch.rand(S, 3, generator=g) * torch.tensor([60.0, 60.0, 3.0])
        pos = (centre[idx] + (torch.rand(idx.numel(), 3, generator=g) - 0.5) * 0.6).float()
        _CLUSTERS[S] = (pos, idx, O.cluster_radius_nn_graph(pos, idx, 30, 0.3, None, True, 3))
    return _CLUSTERS[S]


@pytest.mark.parametrize("S", [8738, 8739])
def test_cluster_radius_nn_graph(S, dev):
    """m + 1 = S * 30 + 1 = 262 141 and 262 171: 64 and 65 scan partials.  Reference and bars:
    tests/test_cluster_graph_gpu.py::test_graph_and_intermediates_match_the_oracle (trimmed
    graph, anchors and edge_index bit-exact, distances rtol 1e-6)."""
    from superpoint_transformer_amd import neighbors as NB
    from superpoint_transformer_amd.ops import segment_reduce
    k_max, gap = 30, 0.3
    pos, idx, (rei, rd, rmid) = clusters(S)
    dpos, didx = pos.to(dev), idx.to(dev)
    lb = lib().lib
    need = lb.spt_cluster_graph_edges_workspace_bytes(S, k_max)

    def run():
        ei, d, mid = NB.cluster_radius_nn_graph(dpos, didx, k_max, gap, None, True, 3, num_clusters=S,
                                                return_intermediate=True)
        return ei, d, mid["trimmed"], mid["anchors"], mid["d_nn"], mid["center_dist"]

    ei, d, trimmed, anchors, d_nn, center_dist = wrapped(dev, run, f"cluster_radius_nn_graph S={S}", [need])
    assert torch.equal(trimmed.cpu(), rmid["trimmed"])
    assert torch.equal(anchors.cpu(), rmid["anchors"])
    assert torch.equal(ei.cpu(), rei)
    assert torch.allclose(d.cpu(), rd, atol=0, rtol=1e-6)
    assert bool((ei[0] < ei[1]).all())

    # the entry point itself with edges / edge_dist cut to the byte: the wrapper's steps up to it
    lo, hi = segment_reduce(dpos, didx, S, "min"), segment_reduce(dpos, didx, S, "max")
    diam = (hi - lo).max(dim=1).values
    nb, dist = NB.knn_1((hi + lo) / 2, k_max, r_max=float(diam.max() + gap))
    nb, dist, r_seg = nb.contiguous(), dist.contiguous(), (diam / 2).contiguous()
    m = S * k_max

    def call(A):
        ws, wsb = A.ws(need)
        edges = A.out(torch.int64, 2, m, label="edges")
        edge_dist = A.out(torch.float32, m, label="edge_dist")
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        ok(lb.spt_cluster_graph_edges(P(nb), P(dist), P(r_seg), S, k_max, gap, 1, P(edges), P(edge_dist),
                                      P(count), P(ws), wsb, stream(dev)), "spt_cluster_graph_edges")
        E = int(count)
        return edges[:, :E], edge_dist[:E]

    edges, edge_dist = c_call(dev, call, f"cluster_graph_edges S={S}")
    same_bits((edges, edge_dist), (trimmed, center_dist), "C ABI against the wrapper")


# ---- sparse_sample: more segments than the sort's partials cover --------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_sparse_sample(masked, dev):
    """n = 300 000 elements in 262 144 segments: the pointer scan runs over 262 145 counts (65
    partials; the sort's region, sized from n, holds 64).  Reference: O.check_sparse_sample(...)
    == [] as in tests/test_segment_gpu.py (pointers bit-exact, the draw held to its contract)."""
    from superpoint_transformer_amd.segment import sparse_sample
    n, num_seg, n_max, n_min, seed = 300_000, 262_144, 4, 1, 17
    g = seeded("sample", masked)
    idx = torch.randint(0, num_seg, (n,), generator=g)
    idx[:5000] = torch.randint(0, 40, (5000,), generator=g)     # some segments above n_max
    idx[-1] = num_seg - 1
    mask = (torch.rand(n, generator=g) < 0.7) if masked else None
    d = idx.to(dev)
    m8 = mask.to(torch.uint8).to(dev) if masked else None
    lb = lib().lib
    need = lb.spt_sparse_sample_workspace_bytes(n, num_seg)

    def call(A):
        ws, wsb = A.ws(need)
        out_ptr = A.out(torch.int64, num_seg + 1, label="out_ptr")
        out_idx = A.out(torch.int64, n, label="out_idx")
        ok(lb.spt_sparse_sample(P(d), n, num_seg, P(m8), n_max, n_min, seed, P(out_ptr), P(out_idx),
                                P(ws), wsb, stream(dev)), "spt_sparse_sample")
        return out_idx[:int(out_ptr[-1])], out_ptr

    s, p = c_call(dev, call, f"sparse_sample masked={masked}")
    assert O.check_sparse_sample(idx, s.cpu(), p.cpu(), n_max, n_min, mask) == []
    w = wrapped(dev, lambda: sparse_sample(d, n_max, n_min, mask=None if mask is None else mask.to(dev),
                                           return_pointers=True, seed=seed, num_segments=num_seg),
                "sparse_sample", [need])
    same_bits(w, (s, p), "wrapper against the C ABI")


# ---- refusal: one byte short ----------------------------------------------------------------------------
def test_cluster_graph_edges_refuses_a_short_workspace(dev):
    S, k = 8739, 30
    m = S * k
    lb = lib().lib
    need = lb.spt_cluster_graph_edges_workspace_bytes(S, k)
    g = torch.Generator().manual_seed(1)
    nb = torch.randint(0, S, (S, k), generator=g).to(dev)
    dist = torch.rand(S, k, generator=g).to(dev)
    r_seg = torch.rand(S, generator=g).to(dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)         # full size behind the short claim
    edges = torch.full((2, m), -7, dtype=torch.int64, device=dev)
    edge_dist = torch.full((m,), -7.0, device=dev)
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = lb.spt_cluster_graph_edges(P(nb), P(dist), P(r_seg), S, k, 0.3, 1, P(edges), P(edge_dist),
                                        P(count), P(ws), need - 1, stream(dev))
    torch.cuda.synchronize(dev)
    assert st != 0 and "workspace" in lib().last_error()
    assert bool((edges == -7).all()) and bool((edge_dist == -7).all()) and int(count) == -7
    with torch.cuda.device(dev):
        ok(lb.spt_cluster_graph_edges(P(nb), P(dist), P(r_seg), S, k, 0.3, 1, P(edges), P(edge_dist),
                                      P(count), P(ws), need, stream(dev)), "spt_cluster_graph_edges")
    assert int(count) > 0


def test_sparse_sample_refuses_a_short_workspace(dev):
    n, num_seg = 300_000, 262_144
    lb = lib().lib
    need = lb.spt_sparse_sample_workspace_bytes(n, num_seg)
    idx = torch.randint(0, num_seg, (n,), generator=torch.Generator().manual_seed(2)).to(dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out_ptr = torch.full((num_seg + 1,), -7, dtype=torch.int64, device=dev)
    out_idx = torch.full((n,), -7, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = lb.spt_sparse_sample(P(idx), n, num_seg, None, 4, 1, 3, P(out_ptr), P(out_idx), P(ws),
                                  need - 1, stream(dev))
    torch.cuda.synchronize(dev)
    assert st != 0 and "workspace" in lib().last_error()
    assert bool((out_ptr == -7).all()) and bool((out_idx == -7).all())
    with torch.cuda.device(dev):
        ok(lb.spt_sparse_sample(P(idx), n, num_seg, None, 4, 1, 3, P(out_ptr), P(out_idx), P(ws), need,
                                stream(dev)), "spt_sparse_sample")
    assert int(out_ptr[-1]) > 0


# ---- cluster select ---------------------------------------------------------------------------------------
def test_cluster_select(dev):
    """Fixture: tests/test_select_gpu.py::test_cluster_select_matches_the_reference (bit-exact against
    the reference's own output); then 4200 clusters over 9000 points with k + 1 = 4097 selected
    sizes to scan, against O.cluster_select (bit-exact)."""
    import test_select_gpu as TS
    from superpoint_transformer_amd.data import Cluster
    lb = lib().lib
    ptr, pts = TS.levels_of("in")[1]["sub"]
    cl_idx = torch.from_numpy(TS.G["cl_idx"])
    c = Cluster(ptr.to(dev), pts.to(dev))
    need = lb.spt_cluster_select_workspace_bytes(cl_idx.numel(), pts.numel(), int(pts.max()) + 1)

    def fixture():
        c2, (idx_sub, sub_super) = c.select(cl_idx.to(dev))
        return c2.pointers, c2.points, idx_sub, sub_super

    got = wrapped(dev, fixture, "Cluster.select (fixture)", [need])
    for t, key in zip(got, ("cl_pointers", "cl_points", "cl_idx_sub", "cl_sub_super")):
        assert torch.equal(t.cpu(), torch.from_numpy(TS.G[key])), key

    g = seeded("cluster_select")
    n_sub, n_cl, k = 9000, 4200, 4096
    si = torch.randint(0, n_cl, (n_sub,), generator=g)
    si[:n_cl] = torch.randperm(n_cl, generator=g)
    ptr, pts = O.cluster_from_index(si, torch.arange(n_sub))
    pick = torch.randperm(n_cl, generator=g)[:k]
    (rptr, rpts), (ridx_sub, rsub_super) = O.cluster_select(ptr, pts, pick)
    c = Cluster(ptr.to(dev), pts.to(dev))
    need = lb.spt_cluster_select_workspace_bytes(k, n_sub, n_sub)

    def synthetic():
        c2, (idx_sub, sub_super) = c.select(pick.to(dev), num_sub=n_sub)
        return c2.pointers, c2.points, idx_sub, sub_super

    got = wrapped(dev, synthetic, "Cluster.select (k + 1 = 4097)", [need])
    for t, r in zip(got, (rptr, rpts, ridx_sub, rsub_super)):
        assert torch.equal(t.cpu(), r)


# ---- grid kNN, its probes, the spatial order ----------------------------------------------------------------
@pytest.mark.parametrize("cell", [None, 0.11])
def test_grid_knn(cell, dev):
    """Reference and bar: tests/test_neighbors_gpu.py::test_grid_knn_is_bit_exact ('mixed', K = 46,
    r = 2: O.frnn_grid_points, indices and f32 distances bit-exact).  ``cell=None`` also runs the
    occupancy probes (spt_grid_count_cells_f32) on exact bitmaps."""
    import test_neighbors_gpu as TN
    from superpoint_transformer_amd import neighbors as NB
    xyz = TN._clouds()["mixed"]
    d = xyz.to(dev)
    if cell is not None:                      # the grid is known: bounding box and cell size
        ext = (xyz.max(0).values - xyz.min(0).values).clamp(min=1e-6).tolist()
        dims = [int(e / cell) + 1 for e in ext]
        assert dims[0] * dims[1] * dims[2] < 1 << 30
    else:                                     # the grid the occupancy probes choose (host code, repeatable)
        _, _, dims = NB._grid_for(d, 2.0, 46, None, self_search=True)
    need = lib().lib.spt_grid_knn_workspace_bytes(xyz.shape[0], dims[0] * dims[1] * dims[2])
    dist, idx = wrapped(dev, lambda: NB.frnn_grid_points(d, d, 46, 2.0, cell_size=cell), f"grid kNN cell={cell}",
                        [need])
    rd, ri = O.frnn_grid_points(xyz, xyz, 46, 2.0)
    assert torch.equal(idx.cpu(), ri) and torch.equal(dist.cpu(), rd)


def cell_ids(xyz, lo, sz, dims):
    """The grid cell of every point, as tests/test_neighbors_gpu.py::
    test_grid_probe_kernels_match_their_torch_expressions restates it (1.0f / sz in f32)."""
    inv = torch.ones((), device=xyz.device) / torch.tensor(sz, device=xyz.device)
    c = ((xyz - torch.tensor(lo, device=xyz.device)) * inv).floor().long()
    for q in range(3):
        c[:, q].clamp_(0, dims[q] - 1)
    return (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]


@pytest.mark.parametrize("sz", [0.5, 0.07])
def test_grid_count_cells(sz, dev):
    """Reference and bar: tests/test_neighbors_gpu.py::
    test_grid_probe_kernels_match_their_torch_expressions (torch.unique of the cell ids, exact)."""
    lb = lib().lib
    xyz = (torch.rand(300_000, 3, generator=seeded("cells")) * torch.tensor([40.0, 25.0, 3.0]) - 7.0).to(dev)
    lo = xyz.min(0).values.tolist()
    ext = (xyz.max(0).values - xyz.min(0).values).tolist()
    dims = [int(e / sz) + 1 for e in ext]
    o3, d3 = (ctypes.c_float * 3)(*lo), (ctypes.c_int32 * 3)(*dims)
    ncells = dims[0] * dims[1] * dims[2]

    def call(A):
        ws, wsb = A.ws(lb.spt_grid_count_cells_workspace_bytes(ncells))
        count = torch.empty(1, dtype=torch.int64, device=dev)
        ok(lb.spt_grid_count_cells_f32(P(xyz), xyz.shape[0], sz, ctypes.cast(o3, ctypes.c_void_p),
                                       ctypes.cast(d3, ctypes.c_void_p), P(count), P(ws), wsb, stream(dev)),
           "spt_grid_count_cells_f32")
        return count

    count = c_call(dev, call, f"grid_count_cells sz={sz}")
    assert int(count) == int(torch.unique(cell_ids(xyz, lo, sz, dims)).numel())


@pytest.mark.parametrize("sz", [1.0, 0.05])
@pytest.mark.parametrize("n", [4096, 4097])
def test_spatial_order(n, sz, dev):
    """order = the stable sort of the cell ids (csr_build on them): torch.sort(stable=True) of the
    ids of test_grid_probe_kernels_match_their_torch_expressions, bit-exact; the wrapper
    (tests/test_neighbors_gpu.py::test_visiting_order_does_not_change_the_features) returns a
    permutation."""
    from superpoint_transformer_amd import neighbors as NB
    lb = lib().lib
    xyz = (torch.rand(n, 3, generator=seeded("order", n)) * torch.tensor([20.0, 12.0, 3.0]) - 4.0).to(dev)
    lo = xyz.min(0).values.tolist()
    ext = (xyz.max(0).values - xyz.min(0).values).tolist()
    dims = [int(e / sz) + 1 for e in ext]
    o3, d3 = (ctypes.c_float * 3)(*lo), (ctypes.c_int32 * 3)(*dims)
    ncells = dims[0] * dims[1] * dims[2]

    def call(A):
        ws, wsb = A.ws(lb.spt_spatial_order_workspace_bytes(n, ncells))
        order = A.out(torch.int32, n, label="order")
        ok(lb.spt_spatial_order(P(xyz), n, sz, ctypes.cast(o3, ctypes.c_void_p),
                                ctypes.cast(d3, ctypes.c_void_p), P(order), P(ws), wsb, stream(dev)),
           "spt_spatial_order")
        return order

    order = c_call(dev, call, f"spatial_order n={n} sz={sz}")
    ref = torch.sort(cell_ids(xyz, lo, sz, dims).cpu(), stable=True).indices
    assert torch.equal(order.cpu().long(), ref)
    box = NB._bbox(xyz)                        # the wrapper's own grid: ~32 points per cell
    _, _, wdims = NB._grid_for(xyz, max(float((box[3:6] - box[0:3]).max()), 1e-3) / 64, 32 / 1.5)
    w = wrapped(dev, lambda: NB.spatial_order(xyz), "spatial_order wrapper",
                [lb.spt_spatial_order_workspace_bytes(n, wdims[0] * wdims[1] * wdims[2])])
    assert torch.equal(torch.sort(w.long()).values, torch.arange(n, device=dev))


# ---- unit sphere norm, graph norm -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,nseg", [(6144, 3), (6147, 3), (5000, 37)])
def test_unit_sphere_norm(n, nseg, dev):
    """Reference and bars: tests/test_norms_gpu.py::test_unit_sphere_norm_random (O.unit_sphere_norm in
    f64: positions within 1e-5 * max(1, |ref|), diameters bit-exact)."""
    import test_norms_gpu as TNo
    from superpoint_transformer_amd import ops
    g = seeded("usn", n, nseg)
    pos = (torch.randn(n, 3, generator=g) * 5 + 20).float()
    idx = torch.arange(n) % nseg                                  # segments of n // nseg rows (+ 1)
    idx = idx[torch.randperm(n, generator=g)]
    w = torch.randint(0, 300, (n,), generator=g)
    need = lib().lib.spt_unit_sphere_workspace_bytes(n, nseg)
    dp, di, dw = pos.to(dev), idx.to(dev), w.to(dev)
    o, d = wrapped(dev, lambda: ops.unit_sphere_norm(dp, di, dw, nseg), f"unit_sphere_norm {n}/{nseg}", [need])
    ro, rd = O.unit_sphere_norm(pos.double(), idx, w, nseg)
    TNo._close(o, ro)
    assert torch.equal(d.cpu(), rd.float())


@pytest.mark.parametrize("r,d,B,slope", [(5000, 32, 3, 0.01), (60000, 128, 40, 0.01)])
def test_graph_norm(r, d, B, slope, dev):
    """Reference and bars: tests/test_norms_gpu.py::test_graph_norm_forward_backward (O.graph_norm in
    f64; output within 1e-5, gradients within 2e-5 of max(1, |ref|); no upstream gradient within
    1e-3 of the LeakyReLU kink)."""
    import test_norms_gpu as TNo
    from superpoint_transformer_amd import ops
    g = seeded("gn", r, d)
    x = (torch.randn(r, d, generator=g) * 2 + 3).float()
    batch = torch.randint(0, B, (r,), generator=g).sort().values
    w, b = torch.randn(d, generator=g).float(), torch.randn(d, generator=g).float()
    a = (1 + 0.3 * torch.randn(d, generator=g)).float()
    gw = torch.randn(r, d, generator=g).float()
    x64 = x.double().requires_grad_()
    p64 = [t.double().requires_grad_() for t in (w, b, a)]
    ref = O.graph_norm(x64, batch, *p64, eps=1e-5, batch_size=B)
    gw = gw * (ref.detach().abs() > 1e-3).float()
    ref = torch.nn.functional.leaky_relu(ref, slope)
    (ref * gw.double()).sum().backward()
    dbatch, dgw = batch.to(dev), gw.to(dev)

    def run():
        xd = x.to(dev).requires_grad_()
        pd = [t.to(dev).requires_grad_() for t in (w, b, a)]
        y = ops.graph_norm(xd, dbatch, *pd, eps=1e-5, num_graphs=B, act_slope=slope)
        (y * dgw).sum().backward()
        return y.detach(), xd.grad, [p.grad for p in pd]

    need = lib().lib.spt_graphnorm_workspace_bytes(r, d, B)
    y, gx, gp = wrapped(dev, run, f"graph_norm {r}x{d} B={B}", [need])
    TNo._close(y, ref.detach(), tol=1e-5)
    TNo._close(gx, x64.grad, tol=2e-5)
    for pg, rg in zip(gp, p64):
        TNo._close(pg, rg.grad, tol=2e-5)


# ---- fused MLP layers, the pool-fused top layer, the sparse statistics ----------------------------------------
@pytest.mark.parametrize("dims,rows,nseg,B,kw", [([12, 32, 64, 128], 40_001, 900, 3, dict(empty=2)),
                                                 ([12, 32, 64], 25_000, 800, 1, dict(neg=7))])
def test_fused_mlp_and_pool(dims, rows, nseg, B, kw, dev):
    """Both routes of MLP -> max-pool: pool-fused (spt_fused_linear_pool_~, spt_fused_linear_~ for the
    layers below, spt_graphnorm_bwd_stats_sparse_~) and materialised (spt_fused_linear_~ for every
    layer, the sparse statistics).  Reference and bars: tests/test_fused_pool_gpu.py::
    test_pool_fused_top_layer_matches_oracle_and_materialised_route (f64 oracle of MLP ->
    scatter_max; values within 2e-5 of max(1, |ref|), gradients no further from the oracle than
    max(2e-4, 3 x the materialised route's error) of the largest entry)."""
    import test_fused_pool_gpu as TP
    lb = lib().lib
    gen = torch.Generator().manual_seed(rows + nseg)
    mlp, x, batch, seg_graph, si, gout = TP._problem(gen, rows, nseg, B, dims, dev, **kw)
    layers = list(zip(dims[:-1], dims[1:]))
    lin = [lb.spt_fused_linear_workspace_bytes(k, n) for k, n in layers]
    sparse = lb.spt_graphnorm_bwd_stats_sparse_workspace_bytes(nseg, dims[-1], B)
    pool = lb.spt_fused_linear_pool_workspace_bytes(dims[-2], dims[-1])
    of, gxf, gpf, _ = wrapped(dev, lambda: TP._run(mlp, x, batch, seg_graph, si, gout, nseg, B, dev, True),
                              "pool-fused route", lin[:-1] + [sparse, pool])
    om, gxm, gpm, _ = wrapped(dev, lambda: TP._run(mlp, x, batch, seg_graph, si, gout, nseg, B, dev, False),
                              "materialised route", lin + [sparse])
    y64, p64, a64, gx64, p64p = TP._oracle(mlp, x, batch, si, gout, nseg)
    assert ((of.double() - p64).abs() / p64.abs().clamp(min=1)).max().item() < 2e-5
    assert ((of - om).abs() / om.abs().clamp(min=1)).max().item() < 1e-5

    def scaled(a, r):
        return float((a.double() - r).abs().max() / r.abs().max().clamp(min=1e-6))
    ef, em = scaled(gxf, gx64), scaled(gxm, gx64)
    assert ef <= max(2e-4, 3 * em), (ef, em)
    for k in gpf:
        r = p64p[k].grad
        ef, em = scaled(gpf[k], r), scaled(gpm[k], r)
        assert ef <= max(2e-4, 3 * em), (k, ef, em)
        assert scaled(gpf[k], gpm[k].double()) < 5e-4, k


# ---- attention backward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,active,deg,H,D,Dv,F,rpe", [(300, 300, 10.0, 16, 4, 4, 32, "kqv"),
                                                       (4000, 250, 10.0, 16, 4, 4, 32, "kqv"),
                                                       (100, 100, 5.0, 8, 8, 8, 32, "")])
def test_edge_attention_backward(n, active, deg, H, D, Dv, F, rpe, dev):
    """Reference and bars: tests/test_attention_gpu.py::test_edge_attention_vs_oracle (O.self_attention in
    f64; |err| <= 1e-5 + 1e-4 |ref| for the output and the input gradients, parameter gradients 2e-5
    of the tensor's largest entry).  The second case is the first one's kind of graph (degree ~11) on
    250 of 4000 nodes, the others without an edge: e ~ 0.7 n, below the e ~ 0.93 n at which the
    target-order layout outgrows the edge-lane one in spt_edge_attn_bwd_ex_workspace_bytes (its
    slope in e changes from 256 to 516 B there); the first case has e ~ 11 n.

    Bit-identity with the generous path is asked where the library promises run-to-run identical
    bits: everything in ``attention_backward_order("source")`` (tests/test_reproducible_gpu.py::
    test_attention_block_in_source_order), the forward output otherwise - the default target
    order and the plain backward sum dk / dv with float atomics (include/spt_hip.h), so two runs
    of theirs differ in the last bit whatever the workspace.  Both orders run on exact
    workspaces and meet the reference."""
    import test_attention_gpu as TA
    from superpoint_transformer_amd import nn as N
    lb = lib().lib
    gen = torch.Generator().manual_seed(n * 7 + H + F)
    dim = H * Dv
    ei = TA._rand_graph(gen, active, deg)
    ei = ei[:, ei[0] != 3]
    ei = ei[:, torch.randperm(ei.shape[1], generator=gen)]
    E = ei.shape[1]
    if active < n:
        assert E < 0.8 * n
        ei = torch.randperm(n, generator=gen)[ei]             # the nodes with edges, spread over all
    blk = N.SelfAttentionBlock(dim, num_heads=H, out_dim=None, qk_dim=D, qk_scale=None, in_rpe_dim=F,
                               k_rpe="k" in rpe, q_rpe="q" in rpe, v_rpe="v" in rpe).to(dev)
    x = torch.randn(n, dim, generator=gen)
    ea = torch.randn(E, F, generator=gen) * 0.5
    gw = torch.randn(n, dim, generator=gen)
    dei, dgw = ei.to(dev), gw.to(dev)

    def run():
        blk.zero_grad(set_to_none=True)
        xd = x.to(dev).requires_grad_()
        ead = ea.to(dev).requires_grad_()
        out = blk(xd, dei, edge_attr=ead)
        (out * dgw).sum().backward()
        return out.detach(), xd.grad, ead.grad, {k: v.grad.clone() for k, v in blk.named_parameters()}

    plain = lb.spt_edge_attn_bwd_workspace_bytes(H, D, Dv, F if rpe else 1)   # no edge features reach the op
    ex = lb.spt_edge_attn_bwd_ex_workspace_bytes(n, E, H, D, Dv, max(F, 1))
    # with edge features, which of the two size functions sizes the backward's scratch depends on
    # the formulation in use; without them it is the plain one
    from superpoint_transformer_amd import precision
    if rpe:
        assert (H, D, Dv, F) == (16, 4, 4, 32)
    results = []
    for order in ((None, "source") if rpe else (None,)):
        with precision.attention_backward_order(order):
            # the edge-lane formulation (built for this shape in the default precision) is what
            # asks for the larger scratch: it must be the one that ran
            el = bool(rpe) and bool(lb.spt_edge_attn_bwd_el_supported(H, D, Dv, F, precision.attention_mode()))
            assert el == bool(rpe)
            results.append(wrapped(dev, run, f"edge attention n={n} e={E} order={order}",
                                   [ex] if el else [plain], (),
                                   bits_of=None if order == "source" else (lambda r: r[0])))

    p = {k: v.detach().cpu().double().requires_grad_() for k, v in blk.named_parameters()}
    x64, ea64 = x.double().requires_grad_(), ea.double().requires_grad_()
    old = O.qk_scale_dg                     # qk_scale=None: (dim / H)^-1/2 * degree^-1/2, as that test states it
    O.qk_scale_dg = lambda s, d_, h_: torch.as_tensor(
        (dim // H) ** -0.5 * (s.bincount(minlength=n).double() ** -0.5)[s].view(-1, 1, 1), dtype=torch.float64)
    try:
        ref = O.self_attention(x64, ei, ea64, p, H, D)
    finally:
        O.qk_scale_dg = old
    (ref * gw.double()).sum().backward()
    for out, gx, gea, gp in results:
        TA._check(out, ref, "out")
        TA._check(gx, x64.grad, "g_x")
        if rpe:
            TA._check(gea, ea64.grad, "g_edge_attr")
        for k in gp:
            TA._check(gp[k], p[k].grad, "g_" + k, rel_to_max=True)


# ---- skinny / narrow linear backward ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [4099, 70_001])
def test_skinny_dw(rows, dev):
    """Reference and bar: tests/test_skinny_linear_gpu.py::test_weight_gradient_kernel_matches_float64
    (f64 G^T X; 4e-6 * sqrt(rows) of the product scale in the default split-bf16 mode)."""
    from superpoint_transformer_amd import ops
    K, N = 64, 192
    g = torch.Generator().manual_seed(rows + K + N)
    x, go = torch.randn(rows, K, generator=g), torch.randn(rows, N, generator=g)
    dx, dgo = x.to(dev), go.to(dev)
    need = lib().lib.spt_skinny_dw_workspace_bytes(K, N)
    gw, gb = wrapped(dev, lambda: ops._skinny_dw(dgo, dx, want_bias=True, mode=1), f"skinny dW rows={rows}", [need])
    rb = go.double().sum(0)
    assert (gb.cpu().double() - rb).abs().max() < 2e-6 * max(rows, 16) ** 0.5 * float(go.abs().max()) + 1e-6 * float(rb.abs().max())
    ref = go.double().t() @ x.double()
    tol = 4e-6 * max(rows, 16) ** 0.5 * float(go.abs().max()) * float(x.abs().max()) + 1e-6 * float(ref.abs().max())
    assert (gw.cpu().double() - ref).abs().max() < tol


@pytest.mark.parametrize("rows", [4099, 70_001])
def test_narrow_linear_backward(rows, dev):
    """Reference and bars: tests/test_skinny_linear_gpu.py::test_narrow_head_linear_autograd_matches_float64
    (f64 torch linear; the wide kernels' bars)."""
    from superpoint_transformer_amd import ops
    K, N = 64, 13
    g = torch.Generator().manual_seed(rows + K + N)
    x0, w0 = torch.randn(rows, K, generator=g), torch.randn(N, K, generator=g) * 0.2
    b0, go = torch.randn(N, generator=g), torch.randn(rows, N, generator=g).to(dev)

    def run():
        x, w, b = (t.to(dev).requires_grad_() for t in (x0, w0, b0))
        y = ops.linear(x, w, b)
        return (y.detach(), *torch.autograd.grad(y, (x, w, b), go))

    need = lib().lib.spt_narrow_linear_bwd_workspace_bytes(K, N)
    y, gx, gw, gb = wrapped(dev, run, f"narrow linear rows={rows}", [need])
    xd, wd, bd = (t.double().requires_grad_() for t in (x0, w0, b0))
    yr = torch.nn.functional.linear(xd, wd, bd)
    rx, rw, rb = torch.autograd.grad(yr, (xd, wd, bd), go.cpu().double())
    gmax, xmax, wmax = float(go.abs().max()), float(x0.abs().max()), float(w0.abs().max())
    assert (y.cpu().double() - yr.detach()).abs().max() < 2e-6 * K * xmax * wmax
    assert (gx.cpu().double() - rx).abs().max() < 2e-6 * N * gmax * wmax + 1e-6
    tol = 2e-6 * rows ** 0.5 * gmax * xmax
    assert (gw.cpu().double() - rw).abs().max() < tol + 1e-6 * float(rw.abs().max())
    assert (gb.cpu().double() - rb).abs().max() < tol + 1e-6 * float(rb.abs().max())


# ---- losses ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [256, 257, 70_001])
def test_cross_entropy(rows, dev):
    """Reference and bars: tests/test_loss_gpu.py::test_cross_entropy_matches_torch (f64 torch; loss 1e-6
    relative, d logits 1e-6 of the largest entry)."""
    from superpoint_transformer_amd import ops
    C = 13
    g = torch.Generator().manual_seed(rows + C)
    z0 = (torch.randn(rows, C, generator=g) * 3).to(dev)
    target = torch.randint(0, C + 1, (rows,), generator=g).to(dev)
    target[0] = 0
    s = torch.tensor(0.37, device=dev)

    def run():
        z = z0.clone().requires_grad_()
        loss = ops.cross_entropy(z, target, ignore_index=C)
        (loss * s).backward()
        return loss.detach(), z.grad

    need = lib().lib.spt_cross_entropy_workspace_bytes(rows)
    loss, grad = wrapped(dev, run, f"cross entropy rows={rows}", [need])
    zd = z0.double().requires_grad_()
    ref = torch.nn.functional.cross_entropy(zd, target, ignore_index=C)
    (ref * s.double()).backward()
    assert abs(float(loss) - float(ref.detach())) <= 1e-6 * max(1.0, abs(float(ref.detach())))
    assert float((grad.double() - zd.grad).abs().max()) <= 1e-6 * float(zd.grad.abs().max()) + 1e-12


@pytest.mark.parametrize("rows", [256, 257, 70_001])
@pytest.mark.parametrize("mode", ["histogram", "dominant"])
def test_histogram_loss(rows, mode, dev):
    """Reference and bars: tests/test_hist_loss_gpu.py::test_histogram_loss_matches_the_closed_form (its f64
    closed forms; loss 1e-6 relative, d logits 1e-6 of the largest entry)."""
    import test_hist_loss_gpu as TH
    from superpoint_transformer_amd import ops
    C = 13
    z0, h, w = TH.make_case(rows, C, True, dev)
    s = torch.tensor(0.37, device=dev)

    def run():
        z = z0.clone().requires_grad_()
        loss = ops.histogram_loss(z, h, weight=w, mode=mode)
        (loss * s).backward()
        return loss.detach(), z.grad

    need = lib().lib.spt_cross_entropy_workspace_bytes(rows)
    loss, grad = wrapped(dev, run, f"histogram loss rows={rows} {mode}", [need])
    zd = z0.double().requires_grad_()
    ref = TH.closed_form(zd, h, w.double(), mode)
    (ref * s.double()).backward()
    TH.check(loss, grad, ref.detach(), zd.grad)


# ---- ground elevation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100_003, 131_041, 262_145])
def test_ground_filters(n, dev):
    """spt_ground_bounds_f32 + spt_ground_trim_f32.  Reference and bar: tests/test_ground_gpu.py::
    test_filters_match_the_restatement (ground_reference.ground_mask, exact indices)."""
    import ground_reference as R
    import test_ground_gpu as TG
    lb = lib().lib
    rng = np.random.default_rng(500 + n)
    pos, _ = R.tilted_cloud(rng, n - n // 3, n // 3, extent=30.0, origin=(1.5, -2.0))
    dpos = TG.on(dev, pos)
    need = [lb.spt_ground_bounds_workspace_bytes(n), lb.spt_ground_trim_workspace_bytes(n)]
    for kw in (dict(z_threshold=0.75), dict(xy_grid=0.3, z_threshold=0.75)):
        def run():
            t = TG.G().ground_mask(dpos, **kw)
            return t.indices(), t.count
        idx, count = wrapped(dev, run, f"ground_mask n={n} {sorted(kw)}", need)
        ref = np.nonzero(R.ground_mask(pos, **kw))[0]
        assert np.array_equal(idx.cpu().numpy(), ref) and int(count) == ref.size


def test_ground_ransac(dev):
    """Reference and bars: tests/test_ground_gpu.py::test_fixture_inlier_counts_for_fixed_samples (counts,
    best hypothesis exact; plane within ground_reference.BOUND_PLANE of the f64 closed form) and
    ::test_generated_cloud_counts_match_the_restatement (64 drawn triplets on 40 011 points)."""
    import ground_reference as R
    import test_ground_gpu as TG
    need = [lib().lib.spt_ground_ransac_workspace_bytes(1)]
    f, r = TG.fixture_case("both"), TG.fixture_reference("both")
    pos = TG.on(dev, f["pos"])
    samples = TG.on(dev, f["samples"])
    trimmed = TG.G().ground_mask(pos, **f["params"])

    def run():
        plane = TG.G().fit_ground_plane(pos, trimmed, samples=samples)
        return plane.counts, plane.status
    counts, status = wrapped(dev, run, "fit_ground_plane (fixture)", need)
    plane = TG.G().fit_ground_plane(pos, trimmed, samples=samples)
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), r["counts"])
    assert plane.best_index == r["best"] and plane.num_refit == int(r["inliers"].sum())
    assert R.relative_deviation(plane.plane, r["plane"]) <= R.BOUND_PLANE
    same_bits(status, plane.status, "status of a third run")

    rng = np.random.default_rng(29)
    cloud, is_ground = R.tilted_cloud(rng, 30_011, 10_000, extent=40.0, origin=(-3.0, 8.0))
    g = np.nonzero(is_ground)[0]
    smp = np.stack([rng.choice(g, 3, replace=False) for _ in range(40)]
                   + [rng.choice(cloud.shape[0], 3, replace=False) for _ in range(24)])
    planes, valid = R.hypothesis_planes(cloud, smp)
    ref_counts, _ = R.score(cloud, planes, valid)
    keep = np.array([R.score(cloud, planes[h:h + 1], valid[h:h + 1])[1] > R.MARGIN for h in range(len(smp))])
    assert keep.sum() >= 40
    dpos, dsmp = TG.on(dev, cloud), TG.on(dev, smp[keep])
    all_points = TG.G().ground_mask(dpos)

    def run2():
        p = TG.G().fit_ground_plane(dpos, all_points, samples=dsmp)
        return p.counts, p.status
    counts, _ = wrapped(dev, run2, "fit_ground_plane (generated cloud)", need)
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), ref_counts[keep])


# ---- point colours --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u8", "f32"])
def test_point_colors(name, dev):
    """Reference and bars: tests/test_point_features_gpu.py::test_colours_against_the_reference (the
    reference's own output: rgb and value bit-exact, hsv / lab within point_features_reference.MARGIN x
    its recorded deviation) and ::test_values_do_not_depend_on_the_route (n = 257, 100 003: a prefix
    is bitwise the dense result)."""
    import point_features_reference as R
    import test_point_features_gpu as TF
    from superpoint_transformer_amd import features
    need = [lib().lib.spt_point_color_workspace_bytes(1)]
    z = TF.golden()
    rgb = torch.from_numpy(z[f"{name}_in"]).to(dev)
    out = wrapped(dev, lambda: features.point_colors(rgb, ("rgb", "hsv", "lab")), f"point_colors {name}", need)
    want = {key: torch.from_numpy(z[f"{name}_{key}"]) for key in R.COLOR_KEYS}
    assert torch.equal(out["rgb"].cpu(), want["rgb"])
    assert torch.equal(out["hsv"][:, 2].cpu(), want["hsv"][:, 2])
    allrgb = np.concatenate([z[f"{s}_rgb"] for s in R.COLOR_SETS])
    for key in ("hsv", "lab"):
        scale = np.abs(getattr(R, key)(allrgb)).max(0)
        got = out[key].cpu().numpy().astype(np.float64)
        dev_ref = np.abs(got - want[key].numpy().astype(np.float64)).max(0) / scale
        assert (dev_ref <= R.MARGIN * np.array(R.REFERENCE_DEVIATION[key])).all(), key
    big, full = TF.big(name, dev)
    for n in (257, 100_003):
        pre = wrapped(dev, lambda: features.point_colors(big[:n]), f"point_colors {name} n={n}", need)
        for key in R.COLOR_KEYS:
            assert TF.same_bits(pre[key], full[key][:n]), key


# ---- partition adjacency: stats, count, fill ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 257, 100_003])
def test_partition_adjacency(n, dev):
    """spt_adjacency_stats (+ regression), spt_adjacency_count, spt_adjacency_fill.  Reference and bars:
    tests/test_adjacency_gpu.py::test_synthetic_tables_match_the_restatement (the f64 restatement
    tests/adjacency_reference.py: graph exact, weights within its measured bounds)."""
    import adjacency_reference as R
    import test_adjacency_gpu as TAd
    lb = lib().lib
    gen = torch.Generator().manual_seed(1000 + n)
    nn, dist = R.random_table(gen, n, 45)
    pos = torch.rand(n, 3, generator=gen) * 10
    r = R.partition_adjacency_reference(nn, dist, 10, 1.0, pos, 1, "mean")
    E = r["edge_index"].shape[1]
    need = [lb.spt_adjacency_stats_workspace_bytes(n), lb.spt_adjacency_count_workspace_bytes(n),
            lb.spt_adjacency_fill_workspace_bytes(n, E)]
    graphs = []

    def run():
        g = TAd.run(dev, nn, dist, 10, 1.0, pos, 1, "mean")
        graphs.append(g)
        return g.edge_index, g.edge_attr, g.source_csr
    wrapped(dev, run, f"partition_adjacency n={n}", need)
    TAd.check_graph(graphs[-1], r, f"n = {n}")
    TAd.check_forward_star(graphs[-1], n)
