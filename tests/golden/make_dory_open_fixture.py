"""Cuts the joint opening proof out of a proof file the reference wrote (`zolt prove --dory` of fibonacci.elf: logs/zolt_proof_dory.bin)
into tests/golden/dory_open_captured.bin.

serializeJoltProofWithDory (src/zkvm/mod.zig:1463-1510) ends a proof with writeDoryProof of open(setup(log_size), bytecode_evals, point)
(src/zkvm/jolt_serialization.zig:148-185), five None bytes for the advice proofs and five usize values (trace length, RAM K, bytecode K,
log_k_chunk, lookups_ra_virtual_log_k_chunk). The proof is found from the END of the file: the 45-byte tail is checked, nu and sigma are
the two u32 before it, and the length follows from them —
    VMV 800 + round count 4 + rounds * (first 1632 + second 960) + final 96 + nu, sigma 8 = 908 + 2592 * max(nu, sigma)
— with the round-count word at proof offset 800 as the cross-check.

    python tests/golden/make_dory_open_fixture.py <reference>/logs/zolt_proof_dory.bin
"""
import os
import struct
import sys

TAIL = bytes(5) + struct.pack("<5Q", 256, 65536, 65536, 4, 16)


def cut(blob):
    if blob[-45:] != TAIL:
        raise SystemExit("the 45-byte tail is not five None bytes and (256, 65536, 65536, 4, 16)")
    nu, sigma = struct.unpack("<2I", blob[-53:-45])
    rounds = max(nu, sigma)
    size = 908 + 2592 * rounds
    proof = blob[-45 - size:-45]
    if struct.unpack("<I", proof[800:804])[0] != rounds:
        raise SystemExit("the round count at proof offset 800 does not match max(nu, sigma)")
    return proof, nu, sigma, len(blob) - 45 - size


def main():
    src = sys.argv[1]
    with open(src, "rb") as f:
        proof, nu, sigma, off = cut(f.read())
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dory_open_captured.bin")
    with open(dst, "wb") as f:
        f.write(proof)
    print(f"nu = {nu}, sigma = {sigma}: {len(proof)} bytes from file offset {off} -> {dst}")


if __name__ == "__main__":
    main()
