"""The model of Fiat-Shamir on the device: the Jolt-compatible Blake2b transcript and the round step of a batched sumcheck on
hashlib.blake2b(digest_size=32) and Python integers. It imports nothing from the library. Field values are canonical integers mod R_MOD;
`limbs` / `unlimbs` move between them and the four-word Montgomery elements the ABI carries. A 128-bit challenge is special: its
Montgomery words are the RAW limbs [0, 0, lo, hi], so its value is (lo 2^128 + hi 2^192) / 2^256.

Also the harness around tests/cpp/blake2b_host.cpp: the kernels' own header (zolt_amd/csrc/blake2b.hip.h) compiled for the host."""
import hashlib
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT = 1 << 256
MONT_INV = pow(MONT, -1, R_MOD)
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 448, 4096)
EVALS_ALL, DERIVE_1, DERIVE_13, QUADRATIC = 0, 1, 2, 3
MAX_INST = 8


def blake(data):
    return hashlib.blake2b(bytes(data), digest_size=32).digest()


def limbs(v):
    """canonical integer -> four Montgomery words"""
    m = v % R_MOD * MONT % R_MOD
    return [(m >> (64 * i)) & (2**64 - 1) for i in range(4)]


def unlimbs(w):
    """four Montgomery words (raw challenge limbs included) -> canonical integer"""
    return sum(int(x) << (64 * i) for i, x in enumerate(w)) * MONT_INV % R_MOD


def message(n, seed=3):
    return bytes((i * 7 + seed + (i >> 8)) & 255 for i in range(n))


class Transcript:
    """src/transcripts/blake2b.zig:25-398"""

    def __init__(self, label=b"Jolt", state=None, n_rounds=0):
        self.state = blake(bytes(label).ljust(32, b"\0")) if state is None else bytes(state)
        self.n_rounds = n_rounds

    def hash_with(self, payload):
        self.state = blake(self.state + bytes(28) + self.n_rounds.to_bytes(4, "big") + bytes(payload))
        self.n_rounds += 1
        return self.state

    def append_message(self, msg):
        self.hash_with(bytes(msg).ljust(32, b"\0"))

    def append_bytes(self, data):
        self.hash_with(data)

    def append_u64(self, x):
        self.hash_with(bytes(24) + int(x).to_bytes(8, "big"))

    def append_scalar(self, v):
        self.hash_with((v % R_MOD).to_bytes(32, "big"))

    def append_scalars(self, vs):
        self.append_message(b"begin_append_vector")
        for v in vs:
            self.append_scalar(v)
        self.append_message(b"end_append_vector")

    def challenge_u128(self):
        return int.from_bytes(self.hash_with(b"")[:16], "little")

    def challenge_scalar_words(self):
        """the RAW limbs [0, 0, lo, hi] of the 125-bit challenge"""
        v = self.challenge_u128() & ((1 << 125) - 1)
        return [0, 0, v & (2**64 - 1), v >> 64]

    def challenge_scalar_full(self):
        """:279-309: the 16 bytes reversed and read little-endian, i.e. their big-endian reading, unmasked"""
        return int.from_bytes(self.hash_with(b"")[:16], "big") % R_MOD


def interpolate3(p):
    """UniPoly.interpolateDegree3: [c0, c1, c2, c3] through p(0..3)"""
    inv6, inv2 = pow(6, -1, R_MOD), pow(2, -1, R_MOD)
    return [p[0] % R_MOD, (-11 * p[0] + 18 * p[1] - 9 * p[2] + 2 * p[3]) * inv6 % R_MOD, (2 * p[0] - 5 * p[1] + 4 * p[2] - p[3]) * inv2 % R_MOD,
            (-p[0] + 3 * p[1] - 3 * p[2] + p[3]) * inv6 % R_MOD]


def next_claim(claim, c0, c2, c3, r):
    """the decompression of generateBatchedProof: c1 from the CLAIM"""
    c1 = (claim - 2 * c0 - c2 - c3) % R_MOD
    return (c0 + c1 * r + c2 * r * r + c3 * r * r * r) % R_MOD


def complete(kind, s, claim):
    s = list(s)
    if kind in (DERIVE_1, DERIVE_13):
        s[1] = (claim - s[0]) % R_MOD
    if kind == DERIVE_13:
        s[3] = (s[0] - 3 * s[1] + 3 * s[2]) % R_MOD
    if kind == QUADRATIC:
        s[3] = (3 * s[2] - 3 * s[1] + s[0]) % R_MOD
    return s


class Batch:
    """setupBatching and the rounds of generateBatchedProof over instances {num_rounds, kind, claim, coeff}"""

    def __init__(self, instances, rule=0):
        self.inst = [dict(i) for i in instances]
        self.rule = rule
        self.M = max(i["num_rounds"] for i in self.inst)
        self.round = 0
        self.claim = 0

    def setup(self, t, sample):
        if sample:
            for i in self.inst:
                t.append_scalar(i["claim"])
            for i in self.inst:
                i["coeff"] = t.challenge_scalar_full()
        self.claim = sum(i["coeff"] * pow(2, self.M - i["num_rounds"], R_MOD) * i["claim"] for i in self.inst) % R_MOD

    def step(self, t, sums):
        """sums[i]: the four values the instance's kernels left (ignored where derived, and for inactive instances)
        -> ([c0, c2, c3], the challenge's raw words)"""
        j, comb, done = self.round, [0, 0, 0, 0], {}
        for n, i in enumerate(self.inst):
            start = self.M - i["num_rounds"]
            if j >= start:
                s = complete(i["kind"], sums[n], i["claim"])
                done[n] = s
                comb = [(c + i["coeff"] * v) % R_MOD for c, v in zip(comb, s)]
            else:
                w = i["coeff"] * i["claim"] * pow(2, start - j - (1 if self.rule == 0 else 0), R_MOD)
                comb = [(c + w) % R_MOD for c in comb]
        c = interpolate3(comb)
        t.append_message(b"UniPoly_begin")
        for v in (c[0], c[2], c[3]):
            t.append_scalar(v)
        t.append_message(b"UniPoly_end")
        rw = t.challenge_scalar_words()
        r = unlimbs(rw)
        self.claim = next_claim(self.claim, c[0], c[2], c[3], r)
        for n, s in done.items():
            ci = interpolate3(s)
            self.inst[n]["claim"] = (ci[0] + ci[1] * r + ci[2] * r * r + ci[3] * r * r * r) % R_MOD
        self.round += 1
        return [c[0], c[2], c[3]], rw


# ---- the host harness
RUN_DT = np.dtype([("claim", "<u8", 4), ("r", "<u8", 4), ("inst_claim", "<u8", (MAX_INST, 4)), ("coeff", "<u8", (MAX_INST, 4)),
                   ("sums", "<u8", (MAX_INST, 16)), ("num_rounds", "<u4", MAX_INST), ("kind", "<u4", MAX_INST), ("k", "<u4"), ("max_rounds", "<u4"),
                   ("round", "<u4"), ("rule", "<u4")])  # zg::FsRunState
OPS = {"init": 0, "import": 1, "bytes": 2, "message": 3, "u64": 4, "scalar": 5, "challenge": 6, "challenge_full": 7}


def compile_host(exe, extra=()):
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", *extra, "-I", os.path.join(ROOT, "zolt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "blake2b_host.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def _run(exe, op, n, payload):
    return subprocess.run([exe], input=f"{op} {n}\n".encode() + payload, capture_output=True, check=True).stdout


def host_hashes(exe, msgs):
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    out = _run(exe, 0, len(msgs), struct.pack(f"<{len(off)}Q", *off) + b"".join(msgs))
    return [out[32 * i:32 * i + 32] for i in range(len(msgs))]


def host_script(exe, script):
    """script: [(op name, payload bytes)] -> [(result words, state bytes, n_rounds)] per record"""
    out = _run(exe, 1, len(script), b"".join(struct.pack("<II", OPS[o], len(p)) + p for o, p in script))
    assert len(out) == 72 * len(script)
    return [(list(struct.unpack("<4Q", out[72 * i:72 * i + 32])), out[72 * i + 32:72 * i + 64], struct.unpack("<Q", out[72 * i + 64:72 * i + 72])[0])
            for i in range(len(script))]


def pack_run(batch):
    S = np.zeros((), dtype=RUN_DT)
    S["k"], S["max_rounds"], S["round"], S["rule"] = len(batch.inst), batch.M, batch.round, batch.rule
    S["claim"] = limbs(batch.claim)
    for n, i in enumerate(batch.inst):
        S["inst_claim"][n], S["coeff"][n] = limbs(i["claim"]), limbs(i.get("coeff") or 0)
        S["num_rounds"][n], S["kind"][n] = i["num_rounds"], i["kind"]
    return S


def host_rounds(exe, batch, t, setup, sums_per_round):
    """the header's setup (0 none, 1 given, 2 sampled) and one step per entry of sums_per_round, from the state of `batch` and `t`
    -> [(FsRunState record, state bytes, n_rounds, log words or None)]: after the setup, then after each round"""
    payload = pack_run(batch).tobytes() + t.state + struct.pack("<Q", t.n_rounds) + struct.pack("<I", setup)
    for sums in sums_per_round:
        a = np.zeros((MAX_INST, 16), dtype="<u8")
        for n, s in enumerate(sums):
            a[n] = sum((limbs(v) for v in s), [])
        payload += a.tobytes()
    out = _run(exe, 2, len(sums_per_round), payload)
    res, pos = [], 0
    for j in range(len(sums_per_round) + 1):
        log = None
        if j:
            log = list(struct.unpack("<16Q", out[pos:pos + 128]))
            pos += 128
        S = np.frombuffer(out[pos:pos + RUN_DT.itemsize], dtype=RUN_DT)[0]
        pos += RUN_DT.itemsize
        res.append((S, out[pos:pos + 32], struct.unpack("<Q", out[pos + 32:pos + 40])[0], log))
        pos += 40
    assert pos == len(out)
    return res


def host_next_claims(exe, records):
    """records: (claim, c0, c2, c3 canonical integers, the challenge's four words) -> next claims (canonical integers)"""
    payload = b"".join(struct.pack("<20Q", *(limbs(c) + limbs(c0) + limbs(c2) + limbs(c3) + [int(x) for x in rw])) for c, c0, c2, c3, rw in records)
    out = _run(exe, 3, len(records), payload)
    return [unlimbs(struct.unpack("<4Q", out[32 * i:32 * i + 32])) for i in range(len(records))]
