"""Instruction budget of the reducing sweep that stores lane words (csrc/kernels_path.h: wta_reduce_pixels), read from the ISA
of the current build (csrc/sgm_engine.s) as tests/test_abi_wta_split.py reads it.  The chained second sweep is bound by its
instruction stream, and the selects it used to do on the scalar unit -- which half of which word is the best d, which halves
are its neighbours -- now run in k_wta_select: what the steady-state block of k_sweep_chain<NP, false, SWEEP_REDUCE> has on
top of the SWEEP_ACCUM block, ALL instructions counted, is capped per pixel."""
from collections import Counter

from test_abi_wta_split import SWEEP_ACCUM, SWEEP_REDUCE, _largest_block


def _blocks(NP):
    acc = Counter(_largest_block(f"k_sweep_chainILi{NP}ELb0ELi{SWEEP_ACCUM}E"))
    red = Counter(_largest_block(f"k_sweep_chainILi{NP}ELb0ELi{SWEEP_REDUCE}E"))
    return acc, red


def _no_spill_traffic(red):
    assert red["v_writelane_b32"] == 0, red
    assert not any(k.startswith("scratch_") for k in red), red
    assert red["s_mul_i32"] <= red["buffer_store_dwordx2"] // 2 and red["s_mul_hi_u32"] <= red["buffer_store_dwordx2"] // 2, red


def test_d256_block_is_at_most_55_instructions_per_pixel_larger():
    """NP = 2, 16 pixels per block.  The form that selected on the scalar unit was 78.75 per pixel larger."""
    acc, red = _blocks(2)
    assert acc["buffer_load_dwordx2"] == 32 and red["buffer_load_dwordx2"] == 32, (acc, red)
    extra = (sum(red.values()) - sum(acc.values())) / 16
    print(f"NP = 2: SWEEP_ACCUM {sum(acc.values())}, SWEEP_REDUCE {sum(red.values())} instructions, +{extra:.2f} per pixel")
    assert extra <= 55, (extra, red)
    # 4 path minima per pixel (as in SWEEP_ACCUM), the minimum of S, and the four words around the best
    assert acc["v_readlane_b32"] == 64 and red["v_readlane_b32"] <= 144, red
    assert red["s_mul_i32"] <= 16 and red["s_mul_hi_u32"] <= 16, red
    _no_spill_traffic(red)


def test_d128_block_is_at_most_40_instructions_per_pixel_larger():
    """NP = 1, 32 pixels per block.  The form that selected on the scalar unit was 49.1 per pixel larger."""
    acc, red = _blocks(1)
    px = red["buffer_load_dword"] // 2
    assert px >= 16 and acc["buffer_load_dword"] == 2 * px and red["buffer_store_dwordx2"] == 2 * px, (acc, red)
    extra = (sum(red.values()) - sum(acc.values())) / px
    print(f"NP = 1, {px} pixels: SWEEP_ACCUM {sum(acc.values())}, SWEEP_REDUCE {sum(red.values())} instructions, +{extra:.2f} per pixel")
    assert extra <= 40, (extra, red)
    # 4 path minima per pixel, the minimum of S, and three words (the lane has one register)
    assert red["v_readlane_b32"] <= (4 + 1 + 3) * px, red
    _no_spill_traffic(red)
