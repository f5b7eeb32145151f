#!/usr/bin/env python3
"""Generates tests/golden/codebooks.json from the reference's own VLC tables: the packed binary-tree tables of
src/player.cpp (player.cpp:59-116) are walked and its prefix-class DCT tables (535-546) re-expanded into
(code, length) -> value lists.  tests/test_codebook_vs_reference.py compares espflix_amd/csrc/mpeg1_codebook.h with them.

    python tests/golden/make_codebook_golden.py <reference tree>/src/player.cpp
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TREE_BOOKS = ("macroblock_address_increment", "macroblock_type_I", "macroblock_type_P", "coded_block_pattern", "motion_vec")


def tree_book(src, name):
    m = re.search(r"const uint32_t " + name + r"\[\d+\] = \{(.*?)\};", src, re.S)
    t = [int(x, 16) for x in re.findall(r"0x[0-9A-Fa-f]+", m.group(1))]
    out = {}

    def rec(state, code, ln):
        v = t[state]
        if (v >> 24) == 0 and state != 0:
            val = v & 0xFFFF
            out[(code, ln)] = val - 0x10000 if val >= 0x8000 else val
            return
        for bit, sh in ((0, 24), (1, 16)):
            nxt = (v >> sh) & 0xFF
            if nxt != 0xFF:
                rec(nxt, (code << 1) | bit, ln + 1)
    rec(0, 0, 0)
    return out


def dct_book(src):
    def arr(name):
        body = re.search(r"const int16_t " + name + r"\[[^\]]*\] =\s*\{(.*?)\};", src, re.S).group(1)
        return [(int(a), int(b)) for a, b in re.findall(r"C\((\d+),(\d+)\)", body)] if name != "t_001" else \
            [(0, 0)] + [(int(a), int(b)) for a, b in re.findall(r"C\((\d+),(\d+)\)", body)]
    ref = {}
    ref[(0b011, 3)] = (1, 1)
    ref[(0b0100, 4)] = (0, 2)
    ref[(0b0101, 4)] = (2, 1)
    t = arr("t_001")
    for i in (1, 2, 3):
        ref[(0b00100 | i, 5)] = t[i]
    for i, rl in enumerate(arr("t_00100")):
        ref[(0b00100000 | i, 8)] = rl
    for i, rl in enumerate(arr("t_0001")):
        ref[(0b000100 | i, 6)] = rl
    for i, rl in enumerate(arr("t_00001")):
        ref[(0b0000100 | i, 7)] = rl
    for i, rl in enumerate(arr("t_0000001")):
        ref[(0b0000001000 | i, 10)] = rl
    big = arr("t_0000X")
    for z in range(5):
        for i in range(16):
            ref[((1 << 4) | i, 12 + z)] = big[z * 16 + i]
    return ref


def main(player_cpp):
    src = open(player_cpp).read()
    out = {"what": "VLC code books of the reference decoder (src/player.cpp), expanded: [code, length, value] for the "
                   "tree books, [code, length, run, level] for the DCT coefficient book (tests/golden/make_codebook_golden.py)"}
    for name in TREE_BOOKS:
        out[name] = sorted([c, l, v] for (c, l), v in tree_book(src, name).items())
    out["dct"] = sorted([c, l, r, lv] for (c, l), (r, lv) in dct_book(src).items())
    path = os.path.join(HERE, "codebooks.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
