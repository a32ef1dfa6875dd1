"""The scan's fast path stages a unit's bytes with buffer_load_dwordx4 ... lds: descriptor and
step offset in SGPRs, one instruction per 1 KiB, no VALU beside it.  That holds only while the
compiler knows the unit's state (unit, skip, fr and what follows from them) to be wave-uniform.
Where it does not, it builds the descriptor in VGPRs and wraps every such load in a waterfall
loop (v_readfirstlane_b32 x4, two v_cmp_eq_u64, s_and_saveexec_b64, the load, s_xor_b64 exec,
s_cbranch_execnz back), keeps the step count in a VGPR and spills.  This compiles the device
code and checks, for both cdc_scan_kernel instances, that no basic block with an LDS-DMA
buffer load also holds a v_readfirstlane_b32 or loops back to itself on EXEC, and that the
narrow form (the flagship path) uses no scratch.  CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
ENDS_BLOCK = ("s_cbranch", "s_branch", "s_setpc", "s_endpgm")
DMA = re.compile(r"^buffer_load_dwordx4\b.*\blds\b")


def functions(text):
    """{name: (body lines, ScratchSize or None)} of an assembly listing; the ScratchSize
    comment of a kernel follows its body, before the next function's label."""
    out, cur = {}, None
    for raw in text.split("\n"):
        m = LABEL.match(raw)
        if m and not m.group(1).startswith((".L", "$")):
            cur = m.group(1)
            out[cur] = [[], None]
            continue
        if cur is None:
            continue
        m = re.match(r"^; ScratchSize: (\d+)", raw)
        if m:
            out[cur][1] = int(m.group(1))
        out[cur][0].append(raw)
    return {k: (v[0], v[1]) for k, v in out.items()}


def basic_blocks(lines):
    """[(label or None, [instructions])]: a block starts at a label and ends after a branch."""
    blocks, label, cur = [], None, []
    for raw in lines:
        m = LABEL.match(raw)
        if m:
            if cur or label:
                blocks.append((label, cur))
            label, cur = m.group(1), []
            continue
        ins = raw.split(";")[0].strip()
        if not ins or ins.startswith("."):
            continue
        cur.append(ins)
        if ins.startswith(ENDS_BLOCK):
            blocks.append((label, cur))
            label, cur = None, []
    if cur or label:
        blocks.append((label, cur))
    return blocks


def dma_findings(lines):
    """(number of LDS-DMA buffer loads, [what is wrong with the blocks that hold them])."""
    loads, bad = 0, []
    for label, ins in basic_blocks(lines):
        n = sum(1 for i in ins if DMA.match(i))
        if not n:
            continue
        loads += n
        if any(i.startswith("v_readfirstlane_b32") for i in ins):
            bad.append("%s: v_readfirstlane_b32 beside an LDS-DMA load" % label)
        last = ins[-1].split()
        if last[0] == "s_cbranch_execnz" and label is not None and last[1] == label:
            bad.append("%s: loops back to itself on EXEC around an LDS-DMA load" % label)
    return loads, bad


@pytest.fixture(scope="module")
def scan_kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    d = tmp_path_factory.mktemp("scan_uniform")
    out = d / "dev.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip",
                    "--cuda-device-only", "-S", os.path.join(ROOT, "pfs_amd/csrc/cdc_kernels.hip"),
                    "-o", str(out)], check=True, capture_output=True, cwd=str(d))
    fns = {k: v for k, v in functions(out.read_text()).items() if "cdc_scan_kernel" in k}
    assert len(fns) == 2 and sum("ILb1E" in k for k in fns) == 1, sorted(fns)  # narrow, wide
    return fns


@pytest.mark.parametrize("wide", [False, True])
def test_no_waterfall_loop_around_an_lds_dma_load(scan_kernels, wide):
    (lines, _), = [v for k, v in scan_kernels.items() if ("ILb1E" in k) == wide]
    loads, bad = dma_findings(lines)
    # 8 per 128-byte step, issued from the prologue and from the step loop
    assert loads >= 16 and loads % 8 == 0, loads
    assert not bad, "\n".join(bad)


def test_narrow_form_uses_no_scratch(scan_kernels):
    (_, scratch), = [v for k, v in scan_kernels.items() if "ILb0E" in k]
    assert scratch == 0, scratch


WATERFALL = """k:
  s_mov_b32 m0, s5
.LBB0_1:
  v_readfirstlane_b32 s8, v2
  v_readfirstlane_b32 s9, v3
  v_readfirstlane_b32 s10, v4
  v_readfirstlane_b32 s11, v5
  v_cmp_eq_u64_e32 vcc, s[8:9], v[2:3]
  s_nop 0
  v_cmp_eq_u64_e64 s[0:1], s[10:11], v[4:5]
  s_and_b64 s[0:1], vcc, s[0:1]
  s_and_saveexec_b64 s[0:1], s[0:1]
  buffer_load_dwordx4 v1, s[8:11], s6 offen lds
  s_xor_b64 exec, exec, s[0:1]
  s_cbranch_execnz .LBB0_1
  s_mov_b64 exec, s[2:3]
  s_endpgm
; ScratchSize: 48
"""

STRAIGHT = """k:
  v_readfirstlane_b32 s8, v2
  s_cbranch_scc0 .LBB0_3
.LBB0_2:
  s_mov_b32 m0, s5
  buffer_load_dwordx4 v1, s[20:23], s6 offen lds
  s_add_i32 m0, s5, 0x400
  buffer_load_dwordx4 v7, s[20:23], s6 offen lds
  buffer_load_dwordx4 v[8:11], v7, s[20:23], 0 offen
  s_cbranch_execnz .LBB0_2
.LBB0_3:
  s_endpgm
; ScratchSize: 0
"""


def test_checker_reports_a_planted_waterfall_loop():
    lines, scratch = functions(WATERFALL)["k"]
    loads, bad = dma_findings(lines)
    assert loads == 1 and scratch == 48
    assert len(bad) == 2 and "v_readfirstlane_b32" in bad[0] and "loops back" in bad[1], bad
    # the loop alone, and the readfirstlane alone, are each reported
    _, bad = dma_findings([l for l in lines if "readfirstlane" not in l])
    assert len(bad) == 1 and "loops back" in bad[0], bad
    _, bad = dma_findings([l for l in lines if "s_cbranch_execnz" not in l])
    assert len(bad) == 1 and "v_readfirstlane_b32" in bad[0], bad
    # straight-line DMA loads pass: a readfirstlane in another block, a plain buffer load and
    # an EXEC branch to the block's own label count only where the block holds the waterfall
    lines, scratch = functions(STRAIGHT)["k"]
    loads, bad = dma_findings(lines)
    assert loads == 2 and scratch == 0 and bad == [".LBB0_2: loops back to itself on EXEC "
                                                   "around an LDS-DMA load"], (loads, bad)
    loads, bad = dma_findings([l.replace("execnz .LBB0_2", "scc1 .LBB0_2") for l in lines])
    assert loads == 2 and not bad, bad
