"""Register and LDS budget of the edge MLP's DMA-staged backward (csrc/fused_mlp_dma.hip,
`fdma::bwd_dma_kernel<32, 32, NW = 4, OCC = 4, LO, !POOLED>`, plain and with the 18 -> 32 layer folded
into it), compiled here to gfx950 assembly with the build's flags, no GPU.

The instances exist for their occupancy: they run on the grid of the register-staged <8, 2> launch,
four workgroups of four waves per CU, and that grid is ONE resident round only at four waves per
SIMD (128 VGPRs), four workgroups per CU in LDS (40 KB each of the CU's 160) and nothing in scratch.
Kernel descriptors only."""
import os
import re
import shutil
import subprocess

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def descriptors(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    from superpoint_transformer_amd import build
    name = "fused_mlp_dma.hip"
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


# <K = 32, N = 32, NW = 4, OCC = 4, LO = true, !POOLED, !S16, FK0>
@pytest.mark.parametrize("fk0", [0, 18], ids=["plain", "fold18"])
def test_edge_dma_backward_is_one_resident_round(descriptors, fk0):
    tag = f"bwd_dma_kernelILi32ELi32ELi4ELi4ELb1ELb0ELb0ELi{fk0}E"
    hit = [(n, d) for n, d in descriptors if tag in n]
    assert len(hit) == 1, [n for n, _ in descriptors]
    name, d = hit[0]
    assert _field(d, "amdhsa_private_segment_fixed_size") == 0, f"{name}: scratch"
    assert _field(d, "amdhsa_next_free_vgpr") <= 128, f"{name}: more than 128 VGPRs"
    assert _field(d, "amdhsa_group_segment_fixed_size") <= 40 * 1024, f"{name}: four workgroups per CU"
