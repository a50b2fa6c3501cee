"""The CPT_* constants of cpppathtracer_amd/_lib.py are a hand copy of include/cpt.h's: every one
of them is held against the header's `#define` or enum value (no GPU needed)."""
import os
import re

from cpppathtracer_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cpt.h")


def header_constants():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"^#define\s+(CPT_\w+)\s+(0[xX][0-9a-fA-F]+|\d+)[uU]?\s*$", text, re.M)
    for body in re.findall(r"\benum\s+\w+\s*\{(.*?)\}", text, re.S):
        found += re.findall(r"\b(CPT_\w+)\s*=\s*(0[xX][0-9a-fA-F]+|\d+)", body)
    return {name: int(value, 0) for name, value in found}


def test_constants_equal_the_headers():
    header = header_constants()
    assert header["CPT_ABI_VERSION"] == 1 and header["CPT_ERR_DEVICE"] == 7 and header["CPT_SCHEDULE_PREVIOUS"] == 0x4000
    mine = {n: v for n, v in vars(_lib).items() if n.startswith("CPT_")}
    assert len(mine) >= 17 and all(type(v) is int for v in mine.values())
    assert {n: header.get(n) for n in mine} == mine
