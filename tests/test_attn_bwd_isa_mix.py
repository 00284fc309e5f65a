"""Instruction budget of the main loop of `to::attn_bwd_to_kernel<3>` (csrc/edge_attn_to.hip), the
target-order attention backward: compiled here to gfx950 assembly with the build's flags, no GPU.

The kernel is bound by instruction issue, not by memory.  Two formatting costs were
removed from it: D reaches its transposed layout as bf16 planes read with `ds_read_b64_tr_b16` (no
word packing and unpacking), and the edge_attr tile is split into bf16 planes once per wave pair.
The hi / lo products that sum over the tile's 16 edges are merged pairwise into 16x16x32 MFMAs by
K-concatenation.  These bounds keep that from regressing silently."""
import collections
import os
import re
import shutil
import subprocess

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


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
    src = os.path.join(build.CSRC, "edge_attn_to.hip")
    out = str(tmp_path_factory.mktemp("isa") / "edge_attn_to.s")
    flags = build.FLAGS + build.PER_FILE_FLAGS.get("edge_attn_to.hip", [])
    r = subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", "-o", out, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def test_main_loop_of_the_f32_backward_keeps_its_instruction_budget(asm):
    cnt = _main_loop_mix(asm, "attn_bwd_to_kernelILi3E")
    mfma = sum(n for op, n in cnt.items() if op.startswith("v_mfma"))
    valu = sum(n for op, n in cnt.items() if op.startswith("v_") and not op.startswith("v_mfma"))
    half = cnt["v_mfma_f32_16x16x16_bf16"]
    assert half <= 12, f"{half} half-rate 16x16x16 MFMAs in the main loop (12 expected: Th Eh per block)"
    assert mfma <= 66, f"{mfma} MFMAs in the main loop"
    assert valu <= 340, f"{valu} VALU instructions in the main loop"
    assert cnt["ds_read_b64_tr_b16"] >= 16, "D and the edge_attr tile are expected to use the transposed read"


def test_both_backward_instances_stay_at_two_waves_per_simd_without_scratch(asm):
    for prec in (3, 1):
        m = re.search(rf"^\s*\.amdhsa_kernel\s+_ZN3spt2to18attn_bwd_to_kernelILi{prec}E.*?\.end_amdhsa_kernel",
                      asm, re.S | re.M)
        assert m, f"kernel descriptor of PREC = {prec} not found"
        d = m.group(0)
        field = lambda k: int(re.search(rf"\.{k}\s+(\d+)", d).group(1))
        assert field("amdhsa_private_segment_fixed_size") == 0, f"PREC {prec}: scratch"
        assert field("amdhsa_next_free_vgpr") <= 256, f"PREC {prec}: more than 256 VGPRs"
        assert field("amdhsa_group_segment_fixed_size") <= 160 * 1024, f"PREC {prec}: LDS"
