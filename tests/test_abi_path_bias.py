"""Instruction budget of the chained sweeps with the clamped and biased path state (csrc/kernels_path.h: path_elem<.., BIAS>),
read from the ISA of the current build (csrc/sgm_engine.s) as tests/test_abi_wta_words.py reads it.  The chained kernels are
bound by their instruction stream.  Per pixel at NP = 2 the biased form drops the explicit min(., P2) of every register of
every direction (-8) and one v_alignbit per direction (-4: the two neighbours a register does not hold come in ONE shifted
word, its own two through the operand selects of the packed minimum), and pays C - B once per register and B - m once per
pixel (+3): -9 vector instructions.  The vector budgets are the parent's counts minus 8 per pixel (1 512 / 1 544 / 1 920 per
16 pixels); as built the blocks hold 1 368 / 1 400 / 1 776.  At NP = 1 (32-pixel blocks, 2 064 / 2 608 on the parent) the same
clamps and alignbits go, and a second half swap restores the operands of the reduction in place of two copies: -8 per
pixel, 7 asked."""
import os
import re
from collections import Counter

import pytest

from test_abi_wta_split import _largest_block, _valu

# all instructions of the 16-pixel blocks as built (DESIGN.md 4.5 quotes the same figures)
AS_BUILT_TOTAL = {0: 1550, 1: 1655, 3: 2414}
VECTOR_BUDGET = {0: 1384, 1: 1416, 3: 1792}
# vector ALU of the 32-pixel NP = 1 blocks of the parent commit (its totals: 2 516 and 3 607)
NP1_PARENT_VECTOR = {1: 2064, 3: 2608}


def _chain(NP, mode):
    return Counter(_largest_block(f"k_sweep_chainILi{NP}ELb0ELi{mode}E"))


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_chained_blocks_vector_budget(mode):
    m = _chain(2, mode)
    print(f"k_sweep_chain<2,false,{mode}>: {sum(m.values())} instructions, {_valu(m)} vector ALU, {m['s_nop']} s_nop")
    assert _valu(m) <= VECTOR_BUDGET[mode], (mode, _valu(m))


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_chained_blocks_total_loads_and_no_spills(mode):
    m = _chain(2, mode)
    total = sum(m.values())
    print(f"k_sweep_chain<2,false,{mode}>: {total} instructions, {_valu(m)} vector ALU, {m['s_nop']} s_nop")
    assert total <= AS_BUILT_TOTAL[mode] + 10, (mode, total)
    if mode == 3:
        assert m["v_readlane_b32"] <= 144, m
    else:
        assert m["v_readlane_b32"] == 64, m
    assert m["v_writelane_b32"] == 0 and not any(k.startswith("scratch_") for k in m), m
    assert m["buffer_load_dwordx2"] == (16 if mode == 0 else 32), m


def test_plain_sweep_blocks_did_not_change():
    """k_sweep keeps the unbiased state and its instruction stream: 1 693 / 1 742 instructions per 16 pixels"""
    for mode, limit in ((0, 1693), (1, 1742)):
        total = len(_largest_block(f"k_sweepILi2ELb0ELi{mode}ELb1E"))
        assert total <= limit, (mode, total)


@pytest.mark.parametrize("mode", [1, 3])
def test_np1_chained_blocks_drop_seven_vector_instructions_per_pixel(mode):
    m = _chain(1, mode)
    px = m["buffer_load_dword"] // 2
    assert px == 32, m
    drop = (NP1_PARENT_VECTOR[mode] - _valu(m)) / px
    print(f"k_sweep_chain<1,false,{mode}>: {sum(m.values())} instructions, {_valu(m)} vector ALU, -{drop:.2f} per pixel")
    assert drop >= 7, (mode, _valu(m), drop)


# scratch bytes per lane of the chained kernels on the parent commit (its resource_usage.txt), by (kernel, NP, PARTIAL, MODE);
# every instantiation not listed had none
PARENT_SCRATCH = {
    ("k_sweep_chain", 1, 1, 0): 12, ("k_sweep_chain", 1, 1, 1): 80, ("k_sweep_chain", 1, 0, 0): 60, ("k_sweep_chain", 1, 0, 1): 60,
    ("k_sweep_chain", 1, 0, 3): 72, ("k_sweep_chain", 2, 1, 1): 12, ("k_sweep_chain", 2, 0, 3): 16, ("k_sweep_chain", 4, 1, 0): 16,
    ("k_sweep_chain", 4, 1, 1): 16, ("k_axis_chain", 1, 1, 1): 24,
}


def test_no_chained_kernel_gained_scratch_or_registers():
    """resource remarks of the build: a chained kernel that had no private segment has none, the others no more than they had
    (the biased form keeps one more scalar alive; the loader and publisher waves derive their row-end conditions per band so
    that nothing is held across the ticket loop), and none goes over the 128 VGPRs that keep four waves per SIMD"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "stereo_reconstruction_cv_amd", "csrc", "resource_usage.txt")).read()
    seen = {}
    for name, vgprs, scratch in re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", txt, flags=re.S):
        m = re.match(r"_ZN3sgm\d+(k_sweep_chain|k_axis_chain)ILi(\d)ELb([01])ELi(\d)EEE", name)
        if m:
            seen[(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))] = (int(vgprs), int(scratch))
    assert len(seen) == 14 + 12, sorted(seen)
    worse = {k: v for k, v in seen.items() if v[1] > PARENT_SCRATCH.get(k, 0) or v[0] > 128}
    assert not worse, worse
    for mode in (0, 1, 3):      # the kernels of the default benchmark
        assert seen[("k_sweep_chain", 2, 0, mode)][1] == 0, seen
