"""GPU: the per-segment sampler ``spt_sparse_sample`` against its host twin
(tests/sampling_reference.py, proven on the host by tests/test_sampling_reference_cpu.py), BIT FOR
BIT on the pointers and on the drawn indices.  The draw is a function of (idx, mask, n_max,
n_min, seed) alone - a counter-based generator, two stable sorts, integer counts - so there is
one right answer and no tolerance anywhere in this file.

What the cases aim at: the full-width (4 x 8 bit) first sort and the segment sort that starts
from the swapped value buffers, at every tile (4096) and wave-chunk (1024) boundary and at the
pass-count thresholds of the segment sort; the stability of the passes under tied keys; the
carry of the count scan past 256 chunks; the f32 count heuristic across its saturation band;
and the consumers of the draw."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import spt_oracle as O
import sampling_reference as S

pytestmark = pytest.mark.gpu

G = load_golden("segment_features.npz")


def t(name):
    return torch.from_numpy(G[name])


def check(dev, idx, n_max, n_min, seed, mask=None, num_segments=None, device_mask=None):
    """Device draw == twin draw; returns the device (samples, ptr) on the host."""
    from superpoint_transformer_amd.segment import sparse_sample
    idx = np.asarray(idx, dtype=np.int64)
    rs, rp = S.sparse_sample(idx, n_max, n_min, seed, mask, num_segments)
    if device_mask is None and mask is not None:
        device_mask = torch.from_numpy(np.asarray(mask)).to(dev)
    s, p = sparse_sample(torch.from_numpy(idx).to(dev), n_max=n_max, n_min=n_min, mask=device_mask,
                         return_pointers=True, seed=seed, num_segments=num_segments)
    s, p = s.cpu(), p.cpu()
    assert s.dtype == torch.int64 and p.dtype == torch.int64
    where = (idx.size, n_max, n_min, seed, num_segments)
    assert torch.equal(p, rp), ("pointers", where, int((p != rp).sum()))
    assert torch.equal(s, rs), ("samples", where, int((s != rs).sum()))
    return s, p


# ---- (a) tile and wave boundaries -------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 + 17])
def test_draw_at_tile_and_wave_boundaries(dev, n):
    # the segment sort goes from one pass to two at bits_for(num_seg + 1) = 9, i.e. num_seg = 256
    for num_seg in (1, 2, 255, 256, 257):
        rng = np.random.default_rng(1000 * num_seg + n)
        idx = rng.integers(0, num_seg, n)
        check(dev, idx, 8, 2, seed=n + num_seg, num_segments=num_seg)
        check(dev, idx, 32, 5, seed=7 * n + num_seg, num_segments=num_seg)


@pytest.mark.parametrize("num_seg", [65535, 65536])
def test_draw_where_the_segment_sort_takes_a_third_pass(dev, num_seg):
    rng = np.random.default_rng(num_seg)
    idx = rng.integers(0, num_seg, 200_003)
    idx[:2] = (0, num_seg - 1)                      # both ends of the id range are populated
    check(dev, idx, 8, 1, seed=num_seg, num_segments=num_seg)


@pytest.mark.parametrize("order", ["sorted", "reversed"])
def test_draw_from_sorted_input(dev, order):
    rng = np.random.default_rng(5)
    idx = np.sort(rng.integers(0, 257, 3 * 4096 + 17))
    check(dev, idx if order == "sorted" else idx[::-1].copy(), 8, 2, seed=31, num_segments=257)


# ---- (b) the whole permutation ----------------------------------------------------------------
def test_whole_permutation_is_the_stable_key_order(dev):
    """One segment drawn entirely: the output is the stable key-sorted order of 2**20 positions,
    tied keys (118 positions with this seed, tests/test_sampling_reference_cpu.py) in ascending
    position - the direct window on the four 8-bit passes."""
    n = S.PERMUTATION_N
    s, p = check(dev, np.zeros(n, dtype=np.int64), n, n, seed=S.PERMUTATION_SEED, num_segments=1)
    assert p.tolist() == [0, n]
    s = s.numpy()
    k = S.keys(S.PERMUTATION_SEED, n)[s]
    tied = k[1:] == k[:-1]
    assert int(tied.sum()) >= 1
    assert bool((k[1:] >= k[:-1]).all()) and bool((s[1:][tied] > s[:-1][tied]).all())


# ---- (c) seeds ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1])
def test_draw_under_extreme_seeds(dev, seed):
    rng = np.random.default_rng(11)
    idx = rng.integers(0, 37, 4097)
    check(dev, idx, 32, 5, seed=seed, num_segments=37)


# ---- (d) masks ---------------------------------------------------------------------------------
def test_draw_under_masks(dev):
    rng = np.random.default_rng(17)
    n, num_seg = 3 * 4096 + 17, 41
    idx = rng.integers(0, num_seg, n)
    mask = rng.random(n) < 0.5
    mask[idx == 3] = False                                    # emptied segments
    mask[idx == 40] = False
    few = np.nonzero(idx == 7)[0]
    mask[few] = False
    mask[few[:3]] = True                                      # 3 kept < n_min = 5
    s, p = check(dev, idx, 32, 5, seed=23, mask=mask, num_segments=num_seg)
    width = (p[1:] - p[:-1]).tolist()
    assert width[3] == 0 and width[40] == 0 and width[7] == 3
    assert sorted(s[p[7]:p[8]].tolist()) == few[:3].tolist()
    # positions instead of a boolean mask: the same draw
    pos = torch.from_numpy(np.nonzero(mask)[0]).to(dev)
    s2, p2 = check(dev, idx, 32, 5, seed=23, mask=mask, num_segments=num_seg, device_mask=pos)
    assert torch.equal(s2, s) and torch.equal(p2, p)
    # everything masked
    s, p = check(dev, idx, 32, 5, seed=23, mask=np.zeros(n, dtype=bool), num_segments=num_seg)
    assert s.numel() == 0 and int(p.max()) == 0


# ---- (e) rows outside the segment range --------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_rows_outside_the_segment_range_are_never_drawn_nor_counted(dev, masked):
    rng = np.random.default_rng(29)
    n, num_seg = 4097, 19
    idx = rng.integers(-3, num_seg + 4, n)                    # negative and >= num_segments rows
    idx[:3] = (-(2 ** 40), 2 ** 40, 2 ** 32 + 5)              # far outside, low 32 bits in range
    mask = rng.random(n) < 0.6 if masked else None
    s, p = check(dev, idx, 8, 2, seed=3, mask=mask, num_segments=num_seg)
    drawn = idx[s.numpy()]
    assert bool(((drawn >= 0) & (drawn < num_seg)).all())


# ---- (f) empty and trailing segments -----------------------------------------------------------
def test_empty_and_trailing_segments(dev):
    rng = np.random.default_rng(37)
    idx = rng.integers(0, 300, 5000)
    idx[(idx % 7) == 0] += 1                                  # holes inside the range
    s, p = check(dev, idx, 8, 2, seed=41, num_segments=300 + 213)
    width = p[1:] - p[:-1]
    assert bool((width[300:] == 0).all()) and bool((width[:300:7] == 0).all())
    check(dev, idx, 8, 0, seed=41, num_segments=300 + 213)    # n_min = 0


# ---- (g) carry of the count scan ---------------------------------------------------------------
@pytest.mark.parametrize("num_seg", [1_048_575, 1_048_577])
def test_count_scan_at_256_and_257_chunks(dev, num_seg):
    """The scan of num_seg + 1 counts takes 256 chunks of 4096 at 1 048 575 segments (one round
    of the partials kernel) and 257 at 1 048 577 (a second round, fed by the carry)."""
    rng = np.random.default_rng(num_seg)
    idx = rng.integers(0, num_seg, 1_200_000)
    idx[-1] = num_seg - 1                                     # the last chunk is populated
    s, p = check(dev, idx, 8, 1, seed=43, num_segments=num_seg)
    assert int(p[-1]) == s.numel() > 0


# ---- (h) counts across the saturation band -----------------------------------------------------
@pytest.mark.parametrize("n_max", [3, 8, 32, 128])
def test_counts_across_the_saturation_band(dev, n_max):
    """One segment of every size in [0, 12 n_max]: above about 8.47 n_max one ulp of tanh moves
    the count between n_max - 1 and n_max; the host f32 value is the correctly rounded one
    (tests/test_sampling_reference_cpu.py)."""
    from superpoint_transformer_amd.segment import sparse_sample
    sizes = np.arange(12 * n_max + 1)
    idx = np.repeat(np.arange(sizes.size), sizes)
    idx = idx[np.random.default_rng(n_max).permutation(idx.size)]
    cnt, _ = S.sample_counts(idx, n_max, 1, None, sizes.size)
    _, p = sparse_sample(torch.from_numpy(idx).to(dev), n_max=n_max, n_min=1, return_pointers=True,
                         seed=n_max, num_segments=sizes.size)
    got = (p[1:] - p[:-1]).cpu().numpy()
    differ = np.nonzero(got != cnt)[0]
    print(f"n_max {n_max}: device and host counts differ at sizes {differ.tolist()}"
          f" (device {got[differ].tolist()}, host {cnt[differ].tolist()})")
    check(dev, idx, n_max, 1, seed=n_max, num_segments=sizes.size)


# ---- (i) consumers -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2 ** 63 + 9])
def test_segment_features_on_their_own_draw_match_the_oracle_on_the_twin_draw(dev, seed):
    """The assertions and bars of tests/test_segment_gpu.py::
    test_segment_features_match_the_reference_on_its_own_samples that judge against the oracle,
    on the sampler's own draw: every segment is judged, the partly sampled ones included."""
    from superpoint_transformer_amd.segment import segment_features
    pos, idx, n = t("scene_pos"), t("scene_idx"), int(G["scene_num_seg"])
    attrs = {"normal": t("scene_normal"), "feat": t("scene_feat")}
    f = segment_features(pos.to(dev), idx.to(dev), n, n_max=32, n_min=5, seed=seed,
                         point_attrs={k: v.to(dev) for k, v in attrs.items()})
    smp, ptr = S.sparse_sample(G["scene_idx"], 32, 5, seed, None, n)
    ref = O.segment_features(pos.double(), idx, n, smp, ptr,
                             point_attrs={k: v.double() for k, v in attrs.items()})
    width = ptr[1:] - ptr[:-1]
    assert int((width < torch.bincount(idx, minlength=n)).sum()) > n // 2    # mostly partly sampled
    ok = width >= 5
    for key in ("linearity", "planarity", "scattering", "curvature", "log_length", "log_surface",
                "log_volume"):
        g = f[key].cpu().double()
        assert torch.allclose(g[ok], ref[key][ok], atol=1e-4), (key, (g - ref[key]).abs().max())
        assert bool((f[key].cpu()[~ok] == 0).all())          # < k_min = 5 samples -> zeroed
    assert torch.allclose(f["log_size"].cpu().double(), ref["log_size"].double(), atol=1e-6)
    assert torch.allclose(f["mean_normal"].cpu().double(), t("scene_mean_normal"), atol=1e-5)
    assert torch.allclose(f["mean_feat"].cpu().double(), ref["mean_feat"], atol=1e-6)
    assert torch.allclose(f["std_feat"].cpu().double(), ref["std_feat"], atol=1e-5)
    assert torch.allclose(f["std_normal"].cpu().double(), ref["std_normal"], atol=1e-5)


def test_get_sampling_and_sample_sub_nodes_equal_the_twin(dev):
    from superpoint_transformer_amd.synthetic import make_raw_nag
    from superpoint_transformer_amd.transforms import NodeSize, SampleSubNodes
    nag = NodeSize(0)(make_raw_nag("R", device=dev))
    for high, n_max, n_min, seed in ((1, 32, 8, 5), (2, 16, 4, 2 ** 64 - 3)):
        si = nag.get_super_index(high, 0).cpu().numpy()
        rs, rp = S.sparse_sample(si, n_max, n_min, seed, None, nag[high].num_nodes)
        s, p = nag.get_sampling(high=high, low=0, n_max=n_max, n_min=n_min, return_pointers=True,
                                seed=seed)
        assert torch.equal(s.cpu(), rs) and torch.equal(p.cpu(), rp)
    mask = torch.arange(nag[0].num_nodes, device=dev) % 3 != 0
    rs, rp = S.sparse_sample(nag.get_super_index(1, 0).cpu().numpy(), 32, 8, 6, mask.cpu().numpy(),
                             nag[1].num_nodes)
    s, p = nag.get_sampling(high=1, low=0, n_max=32, n_min=8, mask=mask, return_pointers=True, seed=6)
    assert torch.equal(s.cpu(), rs) and torch.equal(p.cpu(), rp)
    # SampleSubNodes = select of the twin's draw
    ref_levels = [{k: ((v.pointers.cpu(), v.points.cpu()) if k == "sub" else v.cpu()) for k, v in d}
                  for d in nag]
    rs, _ =S.sparse_sample(nag.get_super_index(1, 0).cpu().numpy(), 32, 8, 5, None,
                            nag[1].num_nodes)
    out = SampleSubNodes(high=1, low=0, n_max=32, n_min=8, seed=5)(nag)
    ref = O.nag_select(ref_levels, 0, rs)
    for d, r in zip(out, ref):
        for k, v in r.items():
            if k == "sub":
                assert torch.equal(d.sub.pointers.cpu(), v[0])
            else:
                assert torch.equal(d[k].cpu(), v), k


def test_sample_edges_equals_the_twin(dev):
    from superpoint_transformer_amd.synthetic import make_raw_nag
    from superpoint_transformer_amd.transforms import SampleEdges
    nag = make_raw_nag("R", device=dev)
    before = {i: (nag[i].edge_index.cpu().clone(), nag[i].edge_attr.cpu().clone()) for i in (1, 2)}
    out = SampleEdges(levels=(1, 2), n_min=2, n_max=4, seed=77)(nag)
    for i in (1, 2):
        ei, ea = before[i]
        rs, _ = S.sparse_sample(ei[0].numpy(), 4, 2, 77, None, out[i].num_nodes)
        assert 0 < rs.numel() < ei.shape[1]                   # the draw does drop edges
        assert torch.equal(out[i].edge_index.cpu(), ei[:, rs])
        assert torch.equal(out[i].edge_attr.cpu(), ea[rs])
