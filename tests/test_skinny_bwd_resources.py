"""Register and LDS budget of the one-pass backward of the attention blocks' Linears
(csrc/skinny_linear.hip, `skinny::skinny_bwd_fused_kernel<NN, PRE, PR>`), compiled
here to gfx950 assembly with the build's flags, no GPU.

The kernel keeps W as bf16 planes and a 64-row macro-tile of gy and x in LDS and a workgroup's share
of the weight-gradient table in accumulators; it hides its global loads behind the products of the
partner wave, so every instance must leave two waves per SIMD: eight-wave workgroups, one per CU at
NN = 192 (<= 256 VGPRs, <= 160 KB of LDS) and two per CU at NN = 64 (<= 128 VGPRs, <= 80 KB), and
nothing in scratch.  Kernel descriptors only."""
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
    name = "skinny_linear.hip"
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


@pytest.mark.parametrize("pr", [3, 1], ids=["split-bf16", "bf16"])
@pytest.mark.parametrize("pre", [0, 1], ids=["plain", "prenorm"])
@pytest.mark.parametrize("nn", [192, 64])
def test_one_pass_backward_leaves_two_waves_per_simd(descriptors, nn, pre, pr):
    tag = f"skinny_bwd_fused_kernelILi{nn}ELb{pre}ELi{pr}E"
    hit = [(n, d) for n, d in descriptors if tag in n]
    assert len(hit) == 1, [n for n, _ in descriptors]
    name, d = hit[0]
    per_cu = 2 if nn == 64 else 1                        # workgroups of 8 waves per CU
    assert _field(d, "amdhsa_private_segment_fixed_size") == 0, f"{name}: scratch"
    vgprs = -(-_field(d, "amdhsa_next_free_vgpr") // 8) * 8
    assert 512 // vgprs >= 2 * per_cu, f"{name}: {vgprs} VGPRs"
    assert _field(d, "amdhsa_group_segment_fixed_size") * per_cu <= 160 * 1024, f"{name}: LDS"
