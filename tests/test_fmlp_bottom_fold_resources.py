"""Register and LDS budget of the folded instance of `fdma::bwd_dma_kernel` (csrc/fused_mlp_dma.hip:
the 32 -> 64 backward that also takes the sums of the 12 -> 32 layer under it),
compiled here to gfx950 assembly with the build's flags, no GPU.

The fold pays only while the upper kernel keeps its occupancy: four waves per SIMD at 128 VGPRs, two
workgroups of eight waves per CU in LDS, nothing in scratch.  The post launch that un-shifts the
sums sits under the 64-register cap of its 1024-thread blocks, also without scratch."""
import os
import re
import shutil
import subprocess

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _descriptors(tmp_path_factory, name):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    from superpoint_transformer_amd import build
    src = os.path.join(build.CSRC, name)
    out = str(tmp_path_factory.mktemp("isa") / (name[:-4] + ".s"))
    flags = build.FLAGS + build.PER_FILE_FLAGS.get(name, [])
    r = subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", "-o", out, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    return re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, re.S | re.M)


def _field(d, k):
    return int(re.search(rf"\.{k}\s+(\d+)", d).group(1))


def test_folded_dma_backward_keeps_its_occupancy_without_scratch(tmp_path_factory):
    descs = _descriptors(tmp_path_factory, "fused_mlp_dma.hip")
    # <K = 32, N = 64, NW = 8, OCC = 4, LO, !POOLED, !S16, FOLD>
    fold = [(n, d) for n, d in descs if "bwd_dma_kernelILi32ELi64ELi8ELi4ELb1ELb0ELb0ELi12E" in n]
    assert len(fold) == 1, [n for n, _ in descs]
    name, d = fold[0]
    assert _field(d, "amdhsa_private_segment_fixed_size") == 0, f"{name}: scratch"
    assert _field(d, "amdhsa_next_free_vgpr") <= 128, f"{name}: more than 128 VGPRs"
    assert _field(d, "amdhsa_group_segment_fixed_size") <= 80 * 1024, f"{name}: two workgroups per CU"


def test_folded_register_staged_backward_keeps_its_occupancy_without_scratch(tmp_path_factory):
    """<K4 = 8, NBK = 2, NEED_GX, NW = 4, LO, ..., FK0 = 18>: the plain instance sits at 132 VGPRs =
    three waves per SIMD (512 / 3 = 170 with the allocation granule: 168); the fold may not cost one."""
    descs = _descriptors(tmp_path_factory, "fused_mlp.hip")
    fold = [(n, d) for n, d in descs if "bwd_kernel_bfILi8ELi2ELb1ELi4ELb1ELb0ELb0ELb0ELb0ELi18E" in n]
    assert len(fold) == 1, [n for n, _ in descs if "bwd_kernel_bf" in n]
    name, d = fold[0]
    assert _field(d, "amdhsa_private_segment_fixed_size") == 0, f"{name}: scratch"
    assert _field(d, "amdhsa_next_free_vgpr") <= 168, f"{name}: fewer than three waves per SIMD"
    assert _field(d, "amdhsa_group_segment_fixed_size") <= 40 * 1024, f"{name}: four workgroups per CU"


def test_post_launch_with_the_fold_blocks_stays_under_its_register_cap(tmp_path_factory):
    descs = _descriptors(tmp_path_factory, "fused_mlp.hip")
    post = [(n, d) for n, d in descs if "bwd_post_kernel" in n]
    assert len(post) == 1
    name, d = post[0]
    assert _field(d, "amdhsa_private_segment_fixed_size") == 0, f"{name}: scratch"
    assert _field(d, "amdhsa_next_free_vgpr") <= 64, f"{name}: more than 64 VGPRs"
