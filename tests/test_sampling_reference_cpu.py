"""CPU proof of the sampler's host twin (tests/sampling_reference.py), the expectation
tests/test_sampling_gpu.py holds the device draw to bit for bit:

  * it honours the sampler's contract and reproduces the REFERENCE'S OWN counts / pointers
    (tests/golden/segment_features.npz, ``sweep_*``) bit for bit;
  * it equals a second, lexicographic restatement of the draw in plain Python integers;
  * its count heuristic (torch f32 on the host) is the correctly rounded one over the whole
    saturation band, so that a device / host difference there is the device's;
  * it draws uniformly on an input of more than three sort tiles whose segments straddle tile and
    wave-chunk boundaries (inclusion and pair frequencies, the chi-square form and 5-sigma bar of
    tests/test_segment_gpu.py::test_sampler_draws_uniformly) - with the bit equality of the GPU
    file this carries the property to the device at multi-tile sizes;
  * the input of the GPU file's whole-permutation case does contain tied keys."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import spt_oracle as O
import augment_reference as A
import sampling_reference as S

G = load_golden("segment_features.npz")


def t(name):
    return torch.from_numpy(G[name])


@pytest.mark.parametrize("case", range(len(G["sweep_cases"])))
def test_twin_honours_the_contract_and_the_reference_counts(case):
    n_max, n_min = G["sweep_cases"][case].tolist()
    idx = t("sweep_idx")
    s, p = S.sparse_sample(G["sweep_idx"], n_max, n_min, seed=case)
    assert torch.equal(p, t(f"sweep_ptr_{case}"))
    assert O.check_sparse_sample(idx, s, p, n_max, n_min) == []


def test_twin_honours_the_contract_and_the_reference_counts_under_a_mask():
    idx, mask = t("sweep_idx"), t("sweep_mask")
    s, p = S.sparse_sample(G["sweep_idx"], 32, 5, seed=11, mask=G["sweep_mask"])
    assert torch.equal(p, t("sweep_ptr_mask"))
    assert O.check_sparse_sample(idx, s, p, 32, 5, mask) == []
    s2, p2 = S.sparse_sample(G["sweep_idx"], 32, 5, seed=11, mask=np.nonzero(G["sweep_mask"])[0])
    assert torch.equal(s2, s) and torch.equal(p2, p)


def lexicographic_draw(idx, n_max, n_min, seed, mask, num_segments):
    """The draw as ONE lexicographic order (bucket, key, position) in Python integers."""
    n = len(idx)
    ok = [0 <= idx[i] < num_segments for i in range(n)]
    keep = [ok[i] and (mask is None or bool(mask[i])) for i in range(n)]
    order = sorted((i for i in range(n) if keep[i]),
                   key=lambda i: (idx[i], A.rand32_scalar(seed & (2 ** 64 - 1), i), i))
    out, ptr = [], [0]
    for s in range(num_segments):
        members = [i for i in order if idx[i] == s]
        size = sum(1 for i in range(n) if ok[i] and idx[i] == s) if mask is not None else len(members)
        want = int(S.heuristic(np.array([size]), n_max)[0])
        take = min(max(want, n_min), size, len(members))
        out += members[:take]
        ptr.append(len(out))
    return out, ptr


@pytest.mark.parametrize("n_max,n_min", [(8, 2), (3, 3), (0, 0), (32, 5)])
def test_twin_equals_the_lexicographic_restatement(n_max, n_min):
    rng = np.random.default_rng(n_max * 7 + n_min)
    n, num_seg = 700, 13
    idx = rng.integers(-2, num_seg + 2, n)                  # rows outside [0, num_seg) included
    idx[idx == 5] = 4                                       # an empty segment
    for mask in (None, rng.random(n) < 0.4):
        for seed in (0, 2 ** 64 - 1, 2 ** 63 + 12345):
            s, p = S.sparse_sample(idx, n_max, n_min, seed, mask, num_seg)
            rs, rp = lexicographic_draw(idx.tolist(), n_max, n_min, seed, mask, num_seg)
            assert p.tolist() == rp and s.tolist() == rs


@pytest.mark.parametrize("n_max", [1, 2, 3, 4, 5, 8, 16, 32, 64, 100, 128, 256, 512])
def test_host_f32_heuristic_is_the_correctly_rounded_one(n_max):
    size = np.arange(12 * n_max + 1)
    assert np.array_equal(S.heuristic(size, n_max), S.correctly_rounded_heuristic(size, n_max))
    assert S.heuristic(size, n_max).max() == n_max          # the band does reach saturation


def test_twin_draws_uniformly_across_sort_tiles():
    # contiguous segments of the INPUT positions; the 48-, 100- and 157-element ones straddle
    # position 1024 (a wave chunk), 4096 and 8192 (sort tiles)
    sizes = [1000, 48, 3000, 100, 4000, 157, 4000]
    n = sum(sizes)
    assert n == 3 * S.SORT_TILE + 17
    edges = np.cumsum([0] + sizes)
    for a, b, cut in ((1, 2, S.WAVE_CHUNK), (3, 4, S.SORT_TILE), (5, 6, 2 * S.SORT_TILE)):
        assert edges[a] < cut < edges[b]
    idx = np.repeat(np.arange(len(sizes)), sizes)
    cnt, _ = S.sample_counts(idx, 8, 2)
    trials = 3000
    hits = np.zeros(n, dtype=np.int64)
    small = 1                                               # pair frequencies of the 48 elements
    pair = np.zeros((sizes[small], sizes[small]))
    for trial in range(trials):
        smp, ptr = S.sparse_sample(idx, 8, 2, seed=1000 + trial)
        smp = smp.numpy()
        hits[smp] += 1
        mine = smp[int(ptr[small]):int(ptr[small + 1])] - edges[small]
        pair[np.ix_(mine, mine)] += 1
    for g, size in enumerate(sizes):
        k = int(cnt[g])
        assert 0 < k < size
        h = hits[idx == g].astype(np.float64)
        p = k / size
        chi2 = float(((h - trials * p) ** 2 / (trials * p * (1 - p))).sum())
        dof = size - 1
        print(f"segment {g}: size {size} k {k} chi2 {chi2:.1f} dof {dof}")
        assert chi2 < dof + 5 * (2 * dof) ** 0.5, (g, chi2, dof)
    k, m = int(cnt[small]), sizes[small]
    ppair = k * (k - 1) / (m * (m - 1))
    off = pair[~np.eye(m, dtype=bool)]
    z = (off - trials * ppair) / (trials * ppair * (1 - ppair)) ** 0.5
    print(f"pairs: max |z| {np.abs(z).max():.2f}")
    assert np.abs(z).max() < 5, z


def test_whole_permutation_case_contains_tied_keys():
    ties = S.tied_keys(S.PERMUTATION_SEED, S.PERMUTATION_N)
    print(f"tied keys among {S.PERMUTATION_N}: {ties}")
    assert ties >= 1
