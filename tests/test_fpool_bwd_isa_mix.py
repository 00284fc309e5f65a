"""Instruction budget of the main loop of `fpool::bwd_pool_kernel<64, 128, true, false, 8>`
(csrc/fused_pool.hip), the backward of the point MLP's top layer with the max-pool inside it:
compiled here to gfx950 assembly with the build's flags, no GPU.

The kernel's product phases were mostly operand formatting: each wave of a pair
staged the whole tile for itself, normalised and split y_prev twice and split a dense S tile that
holds one non-zero per (segment, channel).  Now a pair stages one tile, y_prev and S are written
once as bf16 hi / lo planes (S sparsely), both waves read them as rows and with
`ds_read_b64_tr_b16`, and the three split products of the weight gradient are one 16x16x32 MFMA
by K-concatenation plus one 16x16x16.  These bounds keep that from regressing silently."""
import collections
import os
import re
import shutil
import subprocess

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGSHIP = "bwd_pool_kernelILi64ELi128ELb1ELb0ELi8E"


def _main_loop_mix(text, kernel):
    """Instruction counts of the longest backward branch span of `kernel` (as tools/isa_mix.py)."""
    m = re.search(rf"^(_Z\S*{kernel}\S*):.*?s_endpgm", text, re.S | re.M)
    assert m, f"{kernel} not found"
    lines = [l.strip() for l in m.group(0).split("\n")]
    labels = {}
    for i, l in enumerate(lines):
        lm = re.match(r"^(\.LBB\d+_\d+):", l)
        if lm:
            labels[lm.group(1)] = i
    best = None
    for i, l in enumerate(lines):
        bm = re.match(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if bm and labels.get(bm.group(1), 1 << 30) < i:
            span = i - labels[bm.group(1)]
            if best is None or span > best[0]:
                best = (span, labels[bm.group(1)], i)
    assert best, f"{kernel}: no loop"
    cnt = collections.Counter()
    for l in lines[best[1]:best[2]]:
        if not l or l[0] in ".;" or l.endswith(":"):
            continue
        cnt[l.split()[0]] += 1
    return cnt


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    from superpoint_transformer_amd import build
    src = os.path.join(build.CSRC, "fused_pool.hip")
    out = str(tmp_path_factory.mktemp("isa") / "fused_pool.s")
    flags = build.FLAGS + build.PER_FILE_FLAGS.get("fused_pool.hip", [])
    r = subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", "-o", out, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def test_main_loop_of_the_f32_backward_keeps_its_instruction_budget(asm):
    cnt = _main_loop_mix(asm, FLAGSHIP)
    mfma = sum(n for op, n in cnt.items() if op.startswith("v_mfma"))
    valu = sum(n for op, n in cnt.items() if op.startswith("v_") and not op.startswith("v_mfma"))
    half = cnt["v_mfma_f32_16x16x16_bf16"]
    assert half <= 16, f"{half} half-rate 16x16x16 MFMAs in the main loop (16 expected: sh Xh per block)"
    assert mfma <= 68, f"{mfma} MFMAs in the main loop (32 for gW, 36 for gy)"
    assert cnt["ds_read_b64_tr_b16"] >= 1, "the operands of S^T y_prev are expected to use the transposed read"
    # 548 before the planes; 260 in the kernel as built with them
    assert valu <= 270, f"{valu} VALU instructions in the main loop (260 when this bound was set; 548 before)"


def test_every_backward_instance_fits_registers_and_lds_without_scratch(asm):
    descs = re.findall(r"^\s*\.amdhsa_kernel\s+(_ZN3spt5fpool15bwd_pool_kernel\S*)(.*?)\.end_amdhsa_kernel",
                       asm, re.S | re.M)
    assert len(descs) >= 9, f"{len(descs)} bwd_pool_kernel instances (3 shapes x 3 modes expected)"
    assert any(FLAGSHIP in name for name, _ in descs)
    for name, d in descs:
        field = lambda k: int(re.search(rf"\.{k}\s+(\d+)", d).group(1))
        assert field("amdhsa_private_segment_fixed_size") == 0, f"{name}: scratch"
        assert field("amdhsa_next_free_vgpr") <= 256, f"{name}: more than 256 VGPRs"
        assert field("amdhsa_group_segment_fixed_size") <= 160 * 1024, f"{name}: LDS"
