#!/usr/bin/env python3
"""Extracts the DoryVerifierSetup that the reference's `zolt prove ... --srs` run wrote (logs/zolt_preprocessing.bin, the run of
logs/zolt.log:5530-5541) into tests/golden/dory_verifier_setup_captured.bin: the first 17 904 bytes of that file, which are
DoryVerifierSetup.serialize (src/zkvm/preprocessing.zig:977-1025) for K = 8 — five vectors (delta_1l, delta_1r, delta_2l, delta_2r, chi),
each a u64 count of 9 and nine GT values of 384 bytes, then g1_0 (32), g2_0 (64), h1 (32), h2 (64), ht (384) and max_log_n = 16 as a u64.
The bytecode section that follows is left behind. Data only; run by hand, no test reads the reference tree."""
import hashlib
import os

SRC = os.path.join(os.environ.get("ZOLT_REFERENCE", "/root/reference"), "logs", "zolt_preprocessing.bin")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dory_verifier_setup_captured.bin")
LEVELS, GT_BYTES, LENGTH = 9, 384, 17904
SHA256 = "9137300bccf4ca64796a08be5742f88bc4d7b941a556aac406c1a06629f8d16a"


def main():
    data = open(SRC, "rb").read()
    pos = 0
    for name in ("delta_1l", "delta_1r", "delta_2l", "delta_2r", "chi"):
        count = int.from_bytes(data[pos:pos + 8], "little")
        assert count == LEVELS, (name, count)
        pos += 8 + count * GT_BYTES
    pos += 32 + 64 + 32 + 64 + GT_BYTES  # g1_0, g2_0, h1, h2, ht
    assert pos == 17896 and int.from_bytes(data[pos:pos + 8], "little") == 2 * (LEVELS - 1) == 16
    pos += 8
    assert pos == LENGTH
    cut = data[:LENGTH]
    assert hashlib.sha256(cut).hexdigest() == SHA256
    open(OUT, "wb").write(cut)
    print("wrote", OUT, len(cut), "bytes")


if __name__ == "__main__":
    main()
