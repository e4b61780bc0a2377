"""commitment.py — zolt.poly.commitment: HyperKZG, Dory row commitments.

Part of the zolt_amd.api package (the host mirror of the reference's module API over libzolt_gpu.so); import zolt_amd.api,
which re-exports every name of every part."""
import numpy as np

from .. import lib
from ._base import *  # noqa: F401,F403
from .msm import *  # noqa: F401,F403

# ---- HyperKZG (commit side)
class HyperKZG:
    TAU = 0x12345678  # src/poly/commitment/mod.zig:189 (mock SRS, INSECURE by design)

    class SetupParams:
        def __init__(self, xy, inf, sharded=False, dev=None):
            self.powers_of_tau_g1 = xy
            self.infinity = inf
            self.max_degree = xy.shape[0]
            # device-resident for the whole run (:122-140); sharded=True: one shard per GPU bound by lib.init_devices — commit and
            # batchCommit then go through the one-process multi-GPU entry points (zg_msm_g1_sharded / zg_msm_g1_batch_sharded)
            self.sharded = bool(sharded)
            self._dev = dev if dev is not None else (lib.ShardedBases.upload(xy, inf) if sharded else lib.Bases.upload(xy, inf))

        def deinit(self):
            self._dev.free()

    @staticmethod
    def setup(max_degree, expected_uses=0):
        """powers[i] = scalarMul(G1, tau^i).toAffine() (src/poly/commitment/mod.zig:174-213). expected_uses 1..15: a key that serves one
        proof — no table of multiples (three commits and an opening are fewer MSMs than its break-even); 0: an SRS that lives on."""
        # the powers tau^i (:196-198), the fixed-base batch (every product has the same base: 32 table additions per point instead of
        # double-and-add) and the MSM handle with its table of multiples are built on the device (zg_hyperkzg_setup); the points come back
        # once, for SetupParams.powers_of_tau_g1
        dev, xy, inf = lib.Bases.hyperkzg_setup(generator(), fr_from_int(HyperKZG.TAU), max_degree, expected_uses=expected_uses)
        return HyperKZG.SetupParams(xy, inf, dev=dev)

    @staticmethod
    def commit(params, evals):
        """commit(params, evals) (src/poly/commitment/mod.zig:239-255): empty -> identity; n = min(len, srs)."""
        evals = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, 4)
        if evals.shape[0] == 0:
            return np.zeros(8, dtype=np.uint64), 1
        n = min(evals.shape[0], params.max_degree)
        if params.sharded:
            return params._dev.msm(evals[:n], n=n)
        return params._dev.msm(evals[:n], off=0, n=n)

    @staticmethod
    def commitU64(params, values):
        """commit to the polynomial whose evaluations are F.fromU64 of `values` (machine words) — what commitBytecode / commitMemory /
        commitRegisters build (src/zkvm/mod.zig:1518-1617): the words cross as they are (zg_msm_g1_u64), same commitment bytes"""
        v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
        if v.size == 0:
            return np.zeros(8, dtype=np.uint64), 1
        n = min(v.size, params.max_degree)
        if params.sharded:  # the sharded handle takes field elements
            return HyperKZG.commit(params, lib.field_op(lib.FR, lib.OP_TO_MONT, np.stack([v[:n], np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)], axis=1)))
        return params._dev.msm_u64(v[:n], n=n)

    @staticmethod
    def batchCommit(params, polys):
        """batchCommit (src/poly/commitment/mod.zig:558-570): out[i] = commit(poly_i). Polynomials of equal (clamped)
        length share one zg_msm_g1_batch call, which fuses short vectors into a single launch set."""
        polys = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in polys]
        out = [None] * len(polys)
        groups = {}
        for i, p in enumerate(polys):
            groups.setdefault(min(p.shape[0], params.max_degree), []).append(i)
        for n, idx in groups.items():
            if n == 0 or len(idx) == 1:
                for i in idx:
                    out[i] = HyperKZG.commit(params, polys[i])
            else:
                xy, inf = params._dev.msm_batch([polys[i][:n] for i in idx], n=n)
                for j, i in enumerate(idx):
                    out[i] = (xy[j], int(inf[j]))
        return out

    @staticmethod
    def open(params, evals, point, value):
        """open (src/poly/commitment/mod.zig:261-324): per variable commit(q = hi - lo), fold high half.
        Returns (quotient commitments [(xy, inf)], final_eval)."""
        point = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
        if point.shape[0] == 0:
            return [], np.asarray(value, dtype=np.uint64)
        q, qinf, final = lib.hyperkzg_open(params._dev, evals, point, value)  # whole loop resident on the device
        return [(q[i], int(qinf[i])) for i in range(point.shape[0])], final


    @staticmethod
    def batchOpen(params, polys, point):
        """batchOpen (src/poly/commitment/mod.zig:607-732) -> dict(quotient_commitments [(xy, inf)], evaluations,
        final_eval, batching_challenge); the combination, the evaluations and the fold/commit loop run on the device."""
        point = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
        q, qinf, ev, fin, gam = lib.hyperkzg_batch_open(params._dev, polys, point)
        return {"quotient_commitments": [(q[i], int(qinf[i])) for i in range(q.shape[0])], "evaluations": ev, "final_eval": fin,
                "batching_challenge": gam}


# ---- Dory's wire forms (src/poly/commitment/dory.zig:41-210, src/field/pairing.zig:624-690)
def compressG1(xy, inf):
    """compressG1 (:51-78): x little-endian with the flags in the top two bits of the last byte — 0x40 the identity (all else zero),
    0x80 when y > -y as integers (yIsPositive :162-175: equal counts as positive) -> 32 bytes"""
    if inf:
        return bytes(31) + bytes([0x40])
    xy = np.asarray(xy, dtype=np.uint64).reshape(8)
    x, y = fp_to_int(xy[:4]), fp_to_int(xy[4:])
    out = bytearray(x.to_bytes(32, "little"))
    out[31] = (out[31] & 0x3F) | (0 if y <= (P_MOD - y) % P_MOD else 0x80)
    return bytes(out)


def compressG2(xy, inf):
    """compressG2 (:179-210): x.c0, x.c1 little-endian, flags as compressG1; fp2IsPositive (:320-344) compares c1 first, then c0 -> 64 bytes"""
    if inf:
        return bytes(63) + bytes([0x40])
    w = np.asarray(xy, dtype=np.uint64).reshape(4, 4)
    x0, x1, y0, y1 = (fp_to_int(l) for l in w)
    out = bytearray(x0.to_bytes(32, "little") + x1.to_bytes(32, "little"))
    positive = (y1, y0) <= ((P_MOD - y1) % P_MOD, (P_MOD - y0) % P_MOD)
    out[63] = (out[63] & 0x3F) | (0 if positive else 0x80)
    return bytes(out)


def decompressG1(bytes_list):
    """decompressG1 (:81-120) over a batch of 32-byte records, on the device -> (xy (n, 8), inf (n,)); lib.PointBytesError
    (reason "DecompressionFailed", first_bad) where the reference returns null"""
    return lib.g1_points_from_bytes(b"".join(bytes(b) for b in bytes_list), lib.POINT_BYTES_ARK_COMPRESSED)


def decompressG2(bytes_list):
    """decompressG2 (:214-261) over a batch of 64-byte records -> (xy (n, 16), inf (n,)); an identity is written as G2Point.identity()"""
    return lib.g2_points_from_bytes(b"".join(bytes(b) for b in bytes_list), lib.POINT_BYTES_ARK_COMPRESSED)


class DorySrsError(Exception):
    """InvalidSrsFormat | TruncatedData (Dory.loadFromFile)"""


def gtToBytes(gt):
    """Fp12.toBytes (pairing.zig:624-690) of a 48-word GT element: its twelve Fp values, canonical, little-endian -> 384 bytes"""
    w = np.asarray(gt, dtype=np.uint64).reshape(12, 4)
    return b"".join(fp_to_int(l).to_bytes(32, "little") for l in w)


class DoryProof:
    """DoryProof (:456-536) as the session's message records (include/zolt_gpu.h, "Dory opening (session)"): vmv_message (105 words),
    first_messages [(218,)], second_messages [(148,)], final_message (26,), nu, sigma"""

    def __init__(self, vmv_message, first_messages, second_messages, final_message, nu, sigma):
        self.vmv_message, self.first_messages, self.second_messages = vmv_message, first_messages, second_messages
        self.final_message, self.nu, self.sigma = final_message, nu, sigma

    @staticmethod
    def _g1(rec):
        return compressG1(rec[:8], int(rec[8]) & 1)

    @staticmethod
    def _g2(rec):
        return compressG2(rec[:16], int(rec[16]) & 1)

    def toBytes(self):
        """toBytes (:481-535): VMV, the round count, the first messages, the second messages, the final message, nu, sigma"""
        v = self.vmv_message
        out = gtToBytes(v[0:48]) + gtToBytes(v[48:96]) + self._g1(v[96:105]) + len(self.first_messages).to_bytes(4, "little")
        for m in self.first_messages:
            out += b"".join(gtToBytes(m[48 * k:48 * k + 48]) for k in range(4)) + self._g1(m[192:201]) + self._g2(m[201:218])
        for m in self.second_messages:
            out += gtToBytes(m[0:48]) + gtToBytes(m[48:96]) + self._g1(m[96:105]) + self._g1(m[105:114]) + self._g2(m[114:131]) + self._g2(m[131:148])
        f = self.final_message
        return out + self._g1(f[0:9]) + self._g2(f[9:26]) + int(self.nu).to_bytes(4, "little") + int(self.sigma).to_bytes(4, "little")

    def toArkBytes(self):
        """writeDoryProof (src/zkvm/jolt_serialization.zig:148-185), the form a proof file carries: the VMV message, the round count as a
        u32, the first messages, the second messages, the final message, nu and sigma as u32. The reference's two serialisers write
        the same fields in the same order with the same widths (writeGT = Fp12.toBytes, writeG1Compressed = compressG1, writeG2Compressed
        = compressG2), so this is toBytes under the name of the writer that produced tests/golden/dory_open_captured.bin"""
        return self.toBytes()


class Dory:
    """The data-parallel G1 / G2 / GT / Fr pieces of Dory's commit and open (src/poly/commitment/dory.zig): the row commitments are a
    batch of MSMs over one prefix of g1_vec, the vector-matrix product a weighted column sum, commit their multi-pairing with g2_vec,
    and of openWithTranscript's reduce-and-fold rounds (:1545-1635) the group side — msmG2, the two vector updates in G1 and G2, the
    scalar folds — and the multi-pairings (multiPairG1G2). GT exponentiation, the verifier's GT algebra and the transcript are the
    caller's. openWithTranscript is the whole opening: the pieces above for its inputs, then a device-resident session
    (lib.DoryOpenSession) for the rounds, with the caller's transcript between the messages.
    A G2 vector is a pair (xy (n,16), inf (n,)), a G1 vector (xy (n,8), inf (n,)), a GT element 48 words (lib.multi_pairing)."""

    class SetupParams:
        """SetupParams (:920-998) as far as the prover reads it: g1_vec = (xy (n, 8), inf or None), g2_vec = (xy (n, 16), inf or None)
        with n >= 2^sigma entries each, nu <= sigma. The G1 handle for the row commitments is built on first use."""

        def __init__(self, g1_vec, g2_vec, nu, sigma):
            self.g1_vec, self.g2_vec, self.nu, self.sigma = g1_vec, g2_vec, int(nu), int(sigma)
            self._bases = None

        def g1_bases(self):
            if self._bases is None:
                self._bases = lib.Bases.upload(np.asarray(self.g1_vec[0], dtype=np.uint64).reshape(-1, 8)[:1 << self.sigma],
                                               None if self.g1_vec[1] is None else np.asarray(self.g1_vec[1], dtype=np.uint8)[:1 << self.sigma], expected_uses=4)
            return self._bases

        def deinit(self):
            if self._bases is not None:
                self._bases.free()
                self._bases = None

    URS_SEED = b"Jolt Dory URS seed"  # :953

    # `with Dory.pairing_engine(lib.PAIRING_ENGINE_WAVE):` — every pairing below runs a wavefront per Miller loop and per final
    # exponentiation inside the block (include/zolt_gpu.h, "Pairings (engine)"); the bits are the same
    pairing_engine = staticmethod(lib.pairing_engine)

    @staticmethod
    def setupScalars(max_num_vars):
        """the scalars of setup's generators (:931-979, generateG1Point / generateG2Point :1675-1712) as integers:
        Fr.fromBytes(SHA3-256(seed || u64le(index) || "G1" | "G2")), seed = SHA3-256("Jolt Dory URS seed"), the G2 indices offset by the
        number of columns -> (sigma, nu, [a_c], [b_r])"""
        import hashlib
        sigma = (int(max_num_vars) + 1) // 2
        nu = int(max_num_vars) - sigma
        seed = hashlib.sha3_256(Dory.URS_SEED).digest()

        def scalar(index, tag):
            return int.from_bytes(hashlib.sha3_256(seed + int(index).to_bytes(8, "little") + tag).digest(), "little") % R_MOD

        cols = 1 << sigma
        return sigma, nu, [scalar(i, b"G1") for i in range(cols)], [scalar(i + cols, b"G2") for i in range(1 << nu)]

    @staticmethod
    def setup(max_num_vars):
        """setup (:931-979): 2^sigma G1 and 2^nu G2 generators, sigma = (max_num_vars + 1) / 2, each the group's generator times a hashed
        scalar — one fixed-base batch per group; the hashing is the host's -> SetupParams"""
        sigma, nu, a, b = Dory.setupScalars(max_num_vars)
        g1 = lib.g1_fixed_base_mul_batch(generator(), np.array([fr_from_int(s) for s in a], dtype=np.uint64).reshape(-1, 4))
        g2 = lib.g2_fixed_base_mul_batch(g2_generator(), np.array([fr_from_int(s) for s in b], dtype=np.uint64).reshape(-1, 4))
        return Dory.SetupParams(g1, g2, nu, sigma)

    @staticmethod
    def key(params):
        """the device-resident commitment key of a SetupParams (lib.DoryKey): generators, digit table, MSM handle; the caller frees it"""
        key = lib.DoryKey.create(params.g1_vec, params.g2_vec)
        key.params = params  # what Dory.open reads nu, sigma and the row commitments' handle from
        return key

    SRS_MAGIC = b"JOLT_DORY_SRS_V1"

    @staticmethod
    def parseSrsContainer(data):
        """the container of loadFromFile (:740-822): 16-byte magic | u64 max_num_vars | u64 g1_count | g1_count x 64 B | u64 g2_count |
        g2_count x 128 B | 192 B of h1 / h2 (skipped). Pure host work -> (max_num_vars, g1 bytes, g2 bytes, sigma, nu);
        DorySrsError("InvalidSrsFormat") for a wrong magic, DorySrsError("TruncatedData") for a short file"""
        view = memoryview(data)

        def take(pos, size):
            if pos + size > len(view):
                raise DorySrsError("TruncatedData")
            return view[pos:pos + size], pos + size

        magic, pos = take(0, 16)
        if bytes(magic) != Dory.SRS_MAGIC:
            raise DorySrsError("InvalidSrsFormat")
        word, pos = take(pos, 8)
        max_num_vars = int.from_bytes(word, "little")
        word, pos = take(pos, 8)
        g1, pos = take(pos, 64 * int.from_bytes(word, "little"))
        word, pos = take(pos, 8)
        g2, pos = take(pos, 128 * int.from_bytes(word, "little"))
        take(pos, 64 + 128)
        sigma = (max_num_vars + 1) // 2
        return max_num_vars, g1, g2, sigma, max_num_vars - sigma

    @staticmethod
    def loadFromFile(path_or_bytes):
        """loadFromFile (:752-822): the Jolt-exported Dory SRS of `zolt prove --srs FILE` -> lib.DoryKey with .sigma, .nu and
        .max_num_vars. Both generator vectors are decoded on the device (the arkworks records of :828-924, unchecked as there) and the
        key is built from them where they lie; the caller frees it."""
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            data = path_or_bytes
        else:
            with open(path_or_bytes, "rb") as f:
                data = f.read()
        max_num_vars, g1, g2, sigma, nu = Dory.parseSrsContainer(data)
        key = lib.DoryKey.from_bytes(g1, lib.POINT_BYTES_ARK, g2, lib.POINT_BYTES_ARK)
        key.max_num_vars, key.sigma, key.nu = max_num_vars, sigma, nu
        return key

    @staticmethod
    def batchCommit(key, polys, want_rows=False):
        """commit (:989-1042) for every polynomial of a proof in ONE call over a resident key. polys: a list of
        ("fr", evals (n, 4)) | ("u64", words (n,) [, signs (n,) uint8: 1 = negated]) | ("chunk", column, shift, bits) with column (n,)
        uint64 or (n, 2) uint64 (128-bit little-endian entries) -> gt (k, 48), and with want_rows the row commitments [(xy, inf)] that
        openWithTranscript takes. Chunks that name the same column array cross once."""
        items = []
        for p in polys:
            tag = p[0]
            if tag == "fr":
                items.append((lib.DORY_POLY_FR, np.ascontiguousarray(p[1], dtype=np.uint64).reshape(-1, 4), None, 0, 0))
            elif tag == "u64":
                items.append((lib.DORY_POLY_U64, p[1], p[2] if len(p) > 2 else None, 0, 0))
            elif tag == "chunk":
                col = p[1]
                wide = getattr(col, "ndim", 1) == 2
                items.append((lib.DORY_POLY_CHUNK128 if wide else lib.DORY_POLY_CHUNK64, col, None, int(p[2]), int(p[3])))
            else:
                raise ValueError(f"Dory.batchCommit: unknown polynomial kind {tag!r}")
        return lib.dory_commit_batch(key, items, want_rows=want_rows)

    @staticmethod
    def traceColumnPolys(rd_inc, ram_inc, lookup_index, ram_address, pc, ram_d, bytecode_d, log_k_chunk=4, instruction_d=32):
        """the reference's commitment list in its order (src/zkvm/mod.zig:915-958) from integer columns: RdInc, RamInc as (magnitudes,
        signs), InstructionRa[idx] = chunk idx of the 128-bit lookup index, RamRa of the address column, BytecodeRa of the pc column,
        shift = log_k_chunk * (d - 1 - idx) -> the list batchCommit takes"""
        polys = [("u64",) + tuple(rd_inc), ("u64",) + tuple(ram_inc)]
        for col, d in ((lookup_index, instruction_d), (ram_address, ram_d), (pc, bytecode_d)):
            polys += [("chunk", col, log_k_chunk * (d - 1 - idx), log_k_chunk) for idx in range(d)]
        return polys

    @staticmethod
    def commitTraceColumns(key, rd_inc, ram_inc, lookup_index, ram_address, pc, ram_d, bytecode_d, log_k_chunk=4, instruction_d=32, want_rows=False):
        """every commitment of proveJoltCompatibleWithDoryAndSrsAtAddress (:920-958) in one batch: rd_inc / ram_inc = (magnitudes (T,)
        uint64, signs (T,) uint8), lookup_index (T, 2) uint64, ram_address / pc (T,) uint64 -> 2 + instruction_d + ram_d + bytecode_d GT
        elements in the reference's order"""
        return Dory.batchCommit(key, Dory.traceColumnPolys(rd_inc, ram_inc, lookup_index, ram_address, pc, ram_d, bytecode_d, log_k_chunk, instruction_d),
                                want_rows=want_rows)

    @staticmethod
    def inverseOrOne(x):
        """`x.inverse() orelse F.one()` (:1575, :1613, :1639)"""
        x = np.ascontiguousarray(x, dtype=np.uint64).reshape(4)
        return fr_from_int(1) if not x.any() else lib.field_op(lib.FR, lib.OP_INV, x.reshape(1, 4))[0]

    @staticmethod
    def openWithTranscript(params, evals, point, row_commitments, transcript):
        """openWithTranscript (:1404-1669) -> DoryProof. row_commitments: (xy, inf) or None (computed, :1417-1423); transcript: an object
        with appendGT / appendG1Compressed / appendG2Compressed / challengeScalar (Blake2bTranscript). The vectors cross once, at
        begin; every round then moves two messages out and its challenges in."""
        nu, sigma = params.nu, params.sigma
        rows = row_commitments if row_commitments is not None else Dory.computeRowCommitments(params.g1_bases(), evals, 1 << sigma)
        left_vec, right_vec = Dory.computeEvaluationVectors(point, nu, sigma)
        v_vec = Dory.computeVectorMatrixProduct(evals, left_vec, nu, sigma)
        ses = lib.DoryOpenSession.begin(params.g1_vec, params.g2_vec, rows, v_vec, right_vec, left_vec, nu, sigma)
        try:
            vmv = ses.vmv
            transcript.appendGT(vmv[0:48])
            transcript.appendGT(vmv[48:96])
            transcript.appendG1Compressed((vmv[96:104], int(vmv[104]) & 1))
            firsts, seconds = [], []
            for _ in range(sigma):
                m = ses.first_message()
                firsts.append(m)
                for k in range(4):
                    transcript.appendGT(m[48 * k:48 * k + 48])
                transcript.appendG1Compressed((m[192:200], int(m[200]) & 1))
                transcript.appendG2Compressed((m[201:217], int(m[217]) & 1))
                beta = transcript.challengeScalar()
                m = ses.second_message(beta, Dory.inverseOrOne(beta))
                seconds.append(m)
                transcript.appendGT(m[0:48])
                transcript.appendGT(m[48:96])
                transcript.appendG1Compressed((m[96:104], int(m[104]) & 1))
                transcript.appendG1Compressed((m[105:113], int(m[113]) & 1))
                transcript.appendG2Compressed((m[114:130], int(m[130]) & 1))
                transcript.appendG2Compressed((m[131:147], int(m[147]) & 1))
                alpha = transcript.challengeScalar()
                ses.fold(alpha, Dory.inverseOrOne(alpha))
            gamma = transcript.challengeScalar()
            final = ses.final(gamma, Dory.inverseOrOne(gamma))
            transcript.challengeScalar()  # the final d challenge keeps the transcript in sync (:1658)
        finally:
            ses.close()
        return DoryProof(vmv, firsts, seconds, final, nu, sigma)

    @staticmethod
    def openChallenges(sigma):
        """open's constants in the place of a transcript (:1274, :1316, :1349): beta = round + 1 and alpha = round + 100 per round, then
        gamma = 999, each followed by its `inverse() orelse one` -> (4 sigma + 2, 4), what lib.DoryOpenSession.run takes"""
        out = []
        for c in [v for t in range(sigma) for v in (t + 1, t + 100)] + [999]:
            x = fr_from_int(c)
            out += [x, Dory.inverseOrOne(x)]
        return np.array(out, dtype=np.uint64).reshape(-1, 4)

    @staticmethod
    def open(params_or_key, evals, point):
        """open (:1052-1059) -> DoryProof"""
        return Dory.openWithRowCommitments(params_or_key, evals, point, None)

    @staticmethod
    def openWithRowCommitments(params_or_key, evals, point, row_commitments):
        """openWithRowCommitments (:1062-1378), the opening the prover calls (src/zkvm/mod.zig:1374, :1485) -> DoryProof. Over a resident
        key (Dory.key(params): 2^sigma G1 and 2^nu G2 generators, read where they lie) or over a SetupParams, for which a key is made and
        freed here. row_commitments: (xy, inf) or None (computed, :1073-1080, which needs the key's SetupParams). The rounds run the
        reference's asymmetric schedule; its challenges are constants, so the whole proof is ONE begin and ONE run on the device."""
        if isinstance(params_or_key, lib.DoryKey):
            key, own, params = params_or_key, False, getattr(params_or_key, "params", None)
            n_g1, n_g2 = key.lens()
            nu, sigma = (params.nu, params.sigma) if params is not None else (max(n_g2, 1).bit_length() - 1, n_g1.bit_length() - 1)
        else:
            params = params_or_key
            key, own, nu, sigma = Dory.key(params), True, params.nu, params.sigma
        try:
            if row_commitments is None:
                if params is None:
                    raise ValueError("Dory.open: a key made without Dory.key(params) needs row_commitments")
                row_commitments = Dory.computeRowCommitments(params.g1_bases(), evals, 1 << sigma)
            left_vec, right_vec = Dory.computeEvaluationVectors(point, nu, sigma)
            v_vec = Dory.computeVectorMatrixProduct(evals, left_vec, nu, sigma)
            ses = lib.DoryOpenSession.begin_key(key, row_commitments, v_vec, right_vec, left_vec, nu, sigma)
            try:
                first, second, final = ses.run(Dory.openChallenges(sigma))
            finally:
                ses.close()
        finally:
            if own:
                key.free()
        return DoryProof(ses.vmv, list(first), list(second), final, nu, sigma)

    @staticmethod
    def computeRowCommitments(g1_bases, evals, num_columns):
        """computeRowCommitments (:646-670): g1_bases = a lib.Bases handle over params.g1_vec (resident, like the HyperKZG SRS);
        row r = MSM(g1_vec[0..len(row)], row r of evals). Full rows go through ONE fused launch set (zg_msm_g1_batch), a shorter last
        row is one more MSM over the prefix -> (xy (rows, 8), inf (rows,))"""
        ev = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, 4)
        full, rest = divmod(ev.shape[0], num_columns)
        assert num_columns <= g1_bases.n
        out = np.zeros((full + (1 if rest else 0), 8), dtype=np.uint64)
        inf = np.zeros(out.shape[0], dtype=np.uint8)
        if full:
            out[:full], inf[:full] = g1_bases.msm_batch([ev[r * num_columns:(r + 1) * num_columns] for r in range(full)], n=num_columns)
        if rest:
            xy, i = g1_bases.msm(ev[full * num_columns:], n=rest)
            out[full], inf[full] = xy, i
        return out, inf

    @staticmethod
    def _pairs(g1_vec, g2_vec):
        """the first min(len) entries of a G1 and a G2 vector, flags as arrays (None = no identities)"""
        x1, x2 = np.asarray(g1_vec[0], dtype=np.uint64).reshape(-1, 8), np.asarray(g2_vec[0], dtype=np.uint64).reshape(-1, 16)
        n = min(x1.shape[0], x2.shape[0])
        i1 = np.zeros(n, dtype=np.uint8) if g1_vec[1] is None else np.asarray(g1_vec[1], dtype=np.uint8).reshape(-1)[:n]
        i2 = np.zeros(n, dtype=np.uint8) if g2_vec[1] is None else np.asarray(g2_vec[1], dtype=np.uint8).reshape(-1)[:n]
        return x1[:n], i1, x2[:n], i2

    @staticmethod
    def multiPairBatch(vector_pairs):
        """several multiPairG1G2 (:673-690) in ONE zg_multi_pairing call — a round's six products (:1549-1552, :1587-1588):
        vector_pairs = [(g1_vec, g2_vec)], each product over the min(len) entries of its pair -> (k, 48)"""
        parts = [Dory._pairs(a, b) for a, b in vector_pairs]
        if not parts:
            return np.zeros((0, 48), dtype=np.uint64)
        seg = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in parts])]).astype(np.uint64)
        return lib.multi_pairing(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                                 np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts]), seg)

    @staticmethod
    def multiPairG1G2(g1_vec, g2_vec):
        """multiPairG1G2 (:673-690): prod_i e(g1_vec[i], g2_vec[i]) over min(len) entries, identities skipped -> (48,)"""
        return Dory.multiPairBatch([(g1_vec, g2_vec)])[0]

    @staticmethod
    def commit(g1_bases, g2_vec, evals, num_columns):
        """commit (:1000-1042) for a matrix of num_columns columns: the row commitments (computeRowCommitments), each paired with
        g2_vec[row] and multiplied up — rows past g2_vec are left out (:1030) -> (48,)"""
        rows = Dory.computeRowCommitments(g1_bases, evals, num_columns)
        return Dory.multiPairG1G2(rows, g2_vec)

    @staticmethod
    def multilinearLagrangeBasis(point, out_len=None):
        """multilinearLagrangeBasis (:544-588): the eq table of the point with the index's LOW bit on point[0] — the device's eq table of
        the reversed point; a shorter output is its first entries -> (out_len, 4)"""
        pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
        full = lib.fr_eq_table(np.ascontiguousarray(pt[::-1])) if pt.shape[0] else fr_from_int(1).reshape(1, 4)
        return full if out_len is None else np.ascontiguousarray(full[:out_len])

    @staticmethod
    def computeEvaluationVectors(point, nu, sigma):
        """computeEvaluationVectors (:590-620) -> (left_vec (2^nu, 4), right_vec (2^sigma, 4))"""
        pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
        d = pt.shape[0]
        left, right = np.zeros((1 << nu, 4), dtype=np.uint64), np.zeros((1 << sigma, 4), dtype=np.uint64)
        if d <= sigma:
            right[:1 << d] = Dory.multilinearLagrangeBasis(pt)
            left[0] = fr_from_int(1)
        elif d <= nu + sigma:
            right[:] = Dory.multilinearLagrangeBasis(pt[:sigma])
            left[:1 << (d - sigma)] = Dory.multilinearLagrangeBasis(pt[sigma:])
        else:  # more variables than the matrix has: the row basis is cut at 2^nu entries
            right[:] = Dory.multilinearLagrangeBasis(pt[:sigma])
            left[:] = Dory.multilinearLagrangeBasis(pt[sigma:], 1 << nu)
        return left, right

    @staticmethod
    def computeVectorMatrixProduct(evals, left_vec, nu, sigma):
        """computeVectorMatrixProduct (:622-642): v = L^T M over the 2^nu x 2^sigma matrix of evaluations (zg_fr_weighted_colsum); rows
        past left_vec and entries past evals are zero -> (2^sigma, 4)"""
        rows, cols = 1 << nu, 1 << sigma
        ev = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, 4)
        lv = np.ascontiguousarray(left_vec, dtype=np.uint64).reshape(-1, 4)
        m = np.zeros((rows * cols, 4), dtype=np.uint64)
        m[:min(ev.shape[0], rows * cols)] = ev[:rows * cols]
        w = np.zeros((rows, 4), dtype=np.uint64)
        w[:min(lv.shape[0], rows)] = lv[:rows]
        return lib.fr_weighted_colsum(m, rows, cols, w.reshape(1, rows, 4))[0]

    @staticmethod
    def msmG2(g2_vec, scalars):
        """msmG2 (:693-703): sum_i g2_vec[i].scalarMul(scalars[i]) over min(len) entries -> (xy (16,), inf)"""
        xy, inf = g2_vec
        sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        n = min(np.asarray(xy).size // 16, sc.shape[0])
        return lib.msm_g2(np.asarray(xy).reshape(-1, 16)[:n], None if inf is None else np.asarray(inf)[:n], sc[:n], n=n)

    @staticmethod
    def generateG2Points(scalars, base=None):
        """setup's loop g2_vec[i] = generator.scalarMul(hash_i) (:963-966, generateG2Point :1695-1712) for scalars the caller derived
        (the SHA3 hashing stays with the caller): one fixed-base batch -> (xy (n,16), inf (n,))"""
        return lib.g2_fixed_base_mul_batch(g2_generator() if base is None else base, np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4))

    @staticmethod
    def initV2(g2_0, v_vec, vec_len):
        """v2_work (:1511-1519): v2[i] = g2_vec[0].scalarMul(v_vec[i]) for i < len(v_vec), the identity up to vec_len"""
        v = np.ascontiguousarray(v_vec, dtype=np.uint64).reshape(-1, 4)[:vec_len]
        xy = np.tile(g2_identity(), (vec_len, 1))
        inf = np.ones(vec_len, dtype=np.uint8)
        if v.shape[0]:
            xy[:v.shape[0]], inf[:v.shape[0]] = lib.g2_fixed_base_mul_batch(g2_0, v)
        return xy, inf

    @staticmethod
    def applyFirstChallenge(v1, v2, g1_vec, g2_vec, beta, beta_inv):
        """:1578-1584 over the current_len live entries: v1[i] += beta * g1_vec[i], v2[i] += beta_inv * g2_vec[i] -> (v1, v2)"""
        n = np.asarray(v1[0]).reshape(-1, 8).shape[0]
        new_v1 = lib.g1_axpy_batch(np.asarray(g1_vec[0]).reshape(-1, 8)[:n], None if g1_vec[1] is None else np.asarray(g1_vec[1])[:n], v1[0], v1[1], beta)
        new_v2 = lib.g2_axpy_batch(np.asarray(g2_vec[0]).reshape(-1, 16)[:n], None if g2_vec[1] is None else np.asarray(g2_vec[1])[:n], v2[0], v2[1], beta_inv)
        return new_v1, new_v2

    @staticmethod
    def foldVectors(v1, v2, s1, s2, alpha, alpha_inv):
        """:1615-1632: v1[i] = alpha * v1[i] + v1[i + n2], v2[i] = alpha_inv * v2[i] + v2[i + n2], s1[i] = alpha * s1[i] + s1[i + n2],
        s2[i] = alpha_inv * s2[i] + s2[i + n2] for i < n2 = len / 2 -> the n2 live entries of (v1, v2, s1, s2)"""
        x1, i1 = np.asarray(v1[0]).reshape(-1, 8), np.asarray(v1[1])
        x2, i2 = np.asarray(v2[0]).reshape(-1, 16), np.asarray(v2[1])
        s1 = np.ascontiguousarray(s1, dtype=np.uint64).reshape(-1, 4)
        s2 = np.ascontiguousarray(s2, dtype=np.uint64).reshape(-1, 4)
        n2 = x1.shape[0] // 2
        new_v1 = lib.g1_axpy_batch(x1[:n2], i1[:n2], x1[n2:2 * n2], i1[n2:2 * n2], alpha)
        new_v2 = lib.g2_axpy_batch(x2[:n2], i2[:n2], x2[n2:2 * n2], i2[n2:2 * n2], alpha_inv)
        new_s1 = lib.field_op(lib.FR, lib.OP_ADD, lib.fr_scale(s1[:n2], alpha), s1[n2:2 * n2])
        new_s2 = lib.field_op(lib.FR, lib.OP_ADD, lib.fr_scale(s2[:n2], alpha_inv), s2[n2:2 * n2])
        return new_v1, new_v2, new_s1, new_s2


# ---- the verifier half of the Dory key (src/zkvm/preprocessing.zig:852-1166)
def gtOne():
    """GT.one() as 48 words"""
    out = np.zeros(48, dtype=np.uint64)
    out[:4] = fp_from_int(1)
    return out


def serializeG1(xy, inf):
    """preprocessing.zig's own serializeG1 (:1061-1090), NOT dory.zig's compressG1: x little-endian; bit 62 of the last limb alone for the
    identity; bit 63 set unless y is lexicographicallyLess than -y (:1129-1139: strictly, so y = -y sets it) -> 32 bytes"""
    if inf:
        return bytes(24) + (0x4000000000000000).to_bytes(8, "little")
    xy = np.asarray(xy, dtype=np.uint64).reshape(8)
    x, y = fp_to_int(xy[:4]), fp_to_int(xy[4:])
    return (x | (0 if y < (P_MOD - y) % P_MOD else 1 << 255)).to_bytes(32, "little")


def serializeG2(xy, inf):
    """serializeG2 (:1092-1127): x.c0, x.c1 little-endian, the flags in the last limb of x.c1; lexicographicallyLessFp2 (:1141-1166)
    compares c1 before c0, strictly -> 64 bytes"""
    if inf:
        return bytes(56) + (0x4000000000000000).to_bytes(8, "little")
    w = np.asarray(xy, dtype=np.uint64).reshape(4, 4)
    x0, x1, y0, y1 = (fp_to_int(l) for l in w)
    positive = (y1, y0) < ((P_MOD - y1) % P_MOD, (P_MOD - y0) % P_MOD)
    return x0.to_bytes(32, "little") + (x1 | (0 if positive else 1 << 255)).to_bytes(32, "little")


class DoryVerifierSetup:
    """DoryVerifierSetup (:854-1026) with the reference's field names: delta_1l, delta_1r, delta_2l, delta_2r, chi as (K + 1, 48) GT
    arrays, g1_0 / h1 = (xy (8,), inf), g2_0 / h2 = (xy (16,), inf), ht (48,), max_log_n. Every pairing of fromSRS is one device call
    (lib.dory_verifier_setup[_points]); the copies — delta_1l = delta_2l = (one, chi[:-1]), ht = chi[0] — are made here."""

    def __init__(self, chi, delta_1r, delta_2r, g1_0, g2_0):
        one = gtOne().reshape(1, 48)
        self.chi, self.delta_1r, self.delta_2r = chi, delta_1r, delta_2r
        self.delta_1l = np.concatenate([one, chi[:-1]])  # :905, :926
        self.delta_2l = self.delta_1l.copy()             # :940-945
        self.g1_0, self.g2_0 = g1_0, g2_0                # :965-966
        self.h1, self.h2 = g1_0, g2_0                    # :950-951: the first generators again
        self.ht = chi[0].copy()                          # :957: e(h1, h2) is chi[0]'s pairing
        self.max_log_n = 2 * (chi.shape[0] - 1)          # :970

    @staticmethod
    def _first(vec, words):
        xy = np.asarray(vec[0], dtype=np.uint64).reshape(-1, words)
        return np.ascontiguousarray(xy[0]), 0 if vec[1] is None else int(np.asarray(vec[1]).reshape(-1)[0]) & 1

    @classmethod
    def fromSRS(cls, params_or_key):
        """fromSRS (:889-973) over a Dory.SetupParams (or any object with g1_vec / g2_vec), or over a resident lib.DoryKey"""
        if isinstance(params_or_key, lib.DoryKey):
            key = params_or_key
            chi, d1r, d2r = lib.dory_verifier_setup(key)
            return cls(chi, d1r, d2r, key.g1_0, key.g2_0)
        g1_vec, g2_vec = params_or_key.g1_vec, params_or_key.g2_vec
        chi, d1r, d2r = lib.dory_verifier_setup_points(g1_vec[0], g1_vec[1], g2_vec[0], g2_vec[1])
        return cls(chi, d1r, d2r, cls._first(g1_vec, 8), cls._first(g2_vec, 16))

    def serialize(self):
        """serialize (:977-1025): the five GT vectors, each a u64 count and its elements (serializeGT :1029-1059 = Fp12.toBytes' order),
        g1_0, g2_0, h1, h2, ht, max_log_n as u64 -> bytes"""
        out = b""
        for vec in (self.delta_1l, self.delta_1r, self.delta_2l, self.delta_2r, self.chi):
            out += len(vec).to_bytes(8, "little") + b"".join(gtToBytes(g) for g in vec)
        out += serializeG1(*self.g1_0) + serializeG2(*self.g2_0) + serializeG1(*self.h1) + serializeG2(*self.h2)
        return out + gtToBytes(self.ht) + int(self.max_log_n).to_bytes(8, "little")


__all__ = [_k for _k in dir() if not _k.startswith("__")]  # underscore helpers are shared between the parts too
