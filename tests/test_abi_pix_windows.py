"""CPU-side checks of k_pix's LDS windows on the ISA of the current build (csrc/sgm_engine.s and resource_usage.txt,
by-products of the library build like the checks of tests/test_abi.py): the steady-state block of four columns reads its
disparity windows ready-made from LDS, so what it issues on the vector ALU is the arithmetic and next to nothing else."""
import os
import re
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_reconstruction_cv_amd", "csrc")

# per four columns: Birchfield-Tomasi on packed pairs (7 per pair and plane triple: 2 * 7 * NP per column), gradient +
# (raw >> 2) (2 NP per column), the byte pack (1 per store dword); 18 more are allowed for LDS addresses and the loop
ARITHMETIC = {1: 68, 2: 132, 4: 264}
PARENT = {1: 104, 2: 198, 4: 366}          # the block with the windows shifted in registers, for the record
STORE = {1: "buffer_store_short", 2: "buffer_store_dword", 4: "buffer_store_dwordx2"}


def _largest_block(name_part):
    """instructions of the largest basic block (the unrolled steady-state loop) of the kernel whose mangled name contains name_part"""
    text = open(os.path.join(CSRC, "sgm_engine.s")).read()
    for km in re.finditer(r"^(_Z\w+):\s*; @", text, flags=re.M):
        if name_part not in km.group(1):
            continue
        body = text[km.end():text.index(".Lfunc_end", km.end())].split("\n")
        blocks, cur = [], []
        for l in body:
            if re.match(r"^\.LBB", l):
                blocks.append(cur)
                cur = []
            else:
                cur.append(l)
        blocks.append(cur)
        big = max(blocks, key=len)
        return [l.split()[0] for l in big if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    raise AssertionError(f"no kernel named *{name_part}* in the ISA")


@pytest.mark.parametrize("NP", [1, 2, 4])
def test_block_of_four_columns_is_the_arithmetic(NP):
    m = Counter(_largest_block(f"k_pixILi{NP}E"))
    valu = sum(n for k, n in m.items() if k.startswith("v_"))
    lds = {k: n for k, n in m.items() if k.startswith("ds_")}
    print(f"k_pix<{NP}>: {valu} vector ALU per four columns (arithmetic {ARITHMETIC[NP]}, parent {PARENT[NP]}), "
          f"{sum(m.values())} instructions, LDS {lds}")
    assert m["ds_read_u8"] == 0 and not any(k.startswith("ds_read_u8") for k in m), m      # no byte taps: the windows arrive whole
    assert not any(k.startswith("ds_write") for k in m), m
    assert m[STORE[NP]] == 4 and sum(n for k, n in m.items() if k.startswith("buffer_store")) == 4, m   # four columns
    assert m["s_load_dwordx8"] == 1, m                                                     # their four left-pixel records
    assert valu <= ARITHMETIC[NP] + 18, (valu, m)


def test_no_k_pix_instantiation_has_scratch_or_static_lds():
    """resource_usage.txt: no scratch (the block's 36 window dwords at NP = 2, 60 at NP = 4 stay in registers) and no static
    LDS in front of the dynamic region (the 8-byte reads need its 16-byte-aligned base)"""
    text = open(os.path.join(CSRC, "resource_usage.txt")).read()
    seen = 0
    for km in re.finditer(r"Function Name: (_ZN3sgm5k_pixILi(\d)EEEv\w+)", text):
        rest = text[km.end():]
        nxt = rest.find("Function Name:")
        rec = rest[:nxt if nxt >= 0 else len(rest)]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", rec).group(1))
        vgprs = int(re.search(r"VGPRs: (\d+)", rec).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", rec).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", rec).group(1))
        print(f"k_pix<{km.group(2)}>: {vgprs} VGPRs, occupancy by registers {occ}, scratch {scratch}, static LDS {lds}")
        assert scratch == 0 and lds == 0, km.group(1)
        seen += 1
    assert seen == 3
