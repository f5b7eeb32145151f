"""Exhaustive check of the VLC code books in espflix_amd/csrc/mpeg1_codebook.h against the
reference's own tables: tests/golden/codebooks.json holds them as tests/golden/make_codebook_golden.py
expanded them from the reference's src/player.cpp -- the packed binary-tree tables (player.cpp:59-116)
walked, the prefix-class DCT tables (535-546) re-expanded."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ours(name):
    src = open(os.path.join(ROOT, "espflix_amd", "csrc", "mpeg1_codebook.h")).read()
    body = re.search(r"static const \w+ " + name + r"\[\d+\] = \{(.*?)\};", src, re.S).group(1)
    return [tuple(int(x, 0) for x in m.split(",")) for m in re.findall(r"\{([^{}]*)\}", body)]


def ref_books():
    with open(os.path.join(ROOT, "tests", "golden", "codebooks.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("ours_name,ref_name", [("kMbaCodes", "macroblock_address_increment"), ("kTypeICodes", "macroblock_type_I"),
                                                ("kTypePCodes", "macroblock_type_P"), ("kCbpCodes", "coded_block_pattern"),
                                                ("kMotionCodes", "motion_vec")])
def test_tree_books(ours_name, ref_name):
    mine = {(c, l): v for c, l, v in ours(ours_name)}
    ref = {(c, l): v for c, l, v in ref_books()[ref_name]}
    assert ref and mine == ref


def test_dct_book():
    mine = {(c, l): (r, lv) for c, l, r, lv in ours("kDctCodes")}
    ref = {(c, l): (r, lv) for c, l, r, lv in ref_books()["dct"]}
    assert ref and mine == ref
