#!/usr/bin/env python3
"""Extracts the pairing value the reference records in its own test "pairing generator comparison with jolt"
(src/field/pairing.zig:2200-2263) into tests/golden/pairing_generator_jolt.json: the first 16 bytes of toBytes(e(G1, G2)) as Jolt
computes them (the comment at :2202 and the array at :2256, which must agree), the G1 operand the test builds (:2203) and the leading
bytes of the G2 generator's coordinates it prints for comparison (:2231-2238). Data only."""
import json
import os
import re

SRC = os.path.join(os.environ.get("ZOLT_REFERENCE", "/root/reference"), "src", "field", "pairing.zig")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pairing_generator_jolt.json")


def _bytes(text):
    return bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", text))


def main():
    lines = open(SRC).read().splitlines()
    i0 = next(i for i, l in enumerate(lines) if 'test "pairing generator comparison with jolt"' in l)
    body = lines[i0:i0 + 70]
    comment = next(l for l in body if "first 16 bytes:" in l and l.strip().startswith("//"))
    from_comment = bytes(int(x, 16) for x in comment.split("first 16 bytes:")[1].split())
    from_array = _bytes(next(l for l in body if "const jolt_bytes" in l))
    assert from_comment == from_array and len(from_array) == 16
    g1 = next(l for l in body if "const g1 = G1PointFp" in l)
    assert ".x = Fp.one()" in g1 and ".y = Fp.fromU64(2)" in g1 and ".infinity = false" in g1
    assert any("const g2 = G2Point.generator()" in l for l in body)
    g2 = {name: _bytes(next(l for l in body if f"const jolt_{name} " in l)).hex() for name in ("x_c0", "x_c1", "y_c0", "y_c1")}
    doc = {"source": "reference src/field/pairing.zig:2200-2263 (test \"pairing generator comparison with jolt\"): Jolt's e(G1_gen, G2_gen)",
           "g1": {"x": 1, "y": 2}, "g2": "G2Point.generator()", "g2_generator_le_prefix_hex": g2,
           "layout": "Fp12.toBytes: c0.c0.c0, c0.c0.c1, ... c1.c2.c1, each Fp 32 bytes little-endian, canonical",
           "pairing_to_bytes_first_16_hex": from_array.hex()}
    json.dump(doc, open(OUT, "w"), indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
