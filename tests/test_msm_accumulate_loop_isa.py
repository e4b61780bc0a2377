"""Static guard on everything in the MSM accumulate loop that is NOT a field product (no GPU needed: hipcc cross-compiles for gfx950).

tests/test_msm_accumulate_isa.py pins the ten products of the mixed addition. This test walks the loop of
msm_accumulate_chunk_kernel<false> in the regular build and checks its steady path: the blocks a wave executes when no lane starts
or ends a bucket run and no lane meets the exceptional case of the addition. Found from the control-flow graph, not from block
numbers: of all the ways round the loop that pass through every block of field products and through the row gather, the one with the
fewest vector instructions.

On that path the loop used to spend up to 153 vector instructions around the products: 48 register copies at the loop's end (the 36
accumulator limbs and the 16 row words), 18 moves of the ONE limbs for a case that occurs once per run, 33 for negating y under a
divergent branch, a row gather of six overlapping loads with fix-up moves; and the run-end path read nzlist[r] and starts[.. + 1]
behind a full wait that also drained the row prefetch. The assertions below keep each of those from coming back.
"""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zolt_amd", "csrc")
KERNEL = "_ZN2zg27msm_accumulate_chunk_kernelILb0EEEvPKjS2_S2_S2_PKcjjPc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# Fp29::ONE (fp29.hip.h): the limbs a run start writes into ZZ and ZZZ
ONE = [0x157ccc21, 0x141c2758, 0x185230d3, 0x014c0419, 0x0aa36fb9, 0x1d4240ce, 0x11d54c07, 0x052ac7a8, 0x000dc836]

# Vector instructions of the steady path outside the blocks of field products. The build this test was written against has 47
# (unpacking the row 35, the row's address and the next entry's sign 7, loop counters and branch conditions 5); the ceiling leaves a
# handful of slots for compiler drift. Before: 120, and 153 whenever a lane of the wave subtracted its point. (The exact test for the
# exceptional case is 44 more in either build, in a block that only runs when a 29-bit filter passes: not on the steady path.)
OUTSIDE_VALU_MAX = 52
# ... and of the whole steady path, products included (the digit's sign is folded into R inside the first block of products, where
# it must not hide): 2156 in that build; before 2211, and 2244 whenever a lane subtracted.
PATH_VALU_MAX = 2165


def _hipcc():
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


class Block:
    def __init__(self, label):
        self.label, self.ins, self.succ = label, [], []

    def ops(self):
        return collections.Counter(re.sub(r"_e(32|64)$", "", i.split()[0]) for i in self.ins)

    def valu(self):
        return sum(v for k, v in self.ops().items() if k.startswith("v_"))

    def moves(self):
        return [i for i in self.ins if i.startswith("v_mov_b")]


def _blocks(asm):
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(KERNEL + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith("\t.amdhsa_kernel " + KERNEL))
    blocks = [Block("entry")]
    for l in lines[start + 1:end]:
        m = re.match(r"^(\.LBB\d+_\d+):|^; %bb\.(\d+):", l)
        if m:
            blocks.append(Block(m.group(1) or "bb." + m.group(2)))
            continue
        s = l.split(";")[0].strip()
        if s and not s.startswith("."):
            blocks[-1].ins.append(s)
    index = {b.label: i for i, b in enumerate(blocks)}
    for i, b in enumerate(blocks):
        last = b.ins[-1].split() if b.ins else [""]
        if last[0] == "s_endpgm":
            continue
        if last[0] == "s_branch":
            b.succ = [index[last[1]]]
            continue
        if i + 1 < len(blocks):
            b.succ.append(i + 1)
        if last[0].startswith("s_cbranch"):
            b.succ.append(index[last[1]])
    return blocks


def _reach(blocks, src, allowed=None):
    seen, todo = set(), [src]
    while todo:
        for s in blocks[todo.pop()].succ:
            if s not in seen and (allowed is None or s in allowed):
                seen.add(s)
                todo.append(s)
    return seen


@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    if not _hipcc():
        pytest.skip("hipcc not found")
    out = os.path.join(str(tmp_path_factory.mktemp("loop_isa")), "regular.s")
    cmd = [_hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I" + CSRC,
           os.path.join(CSRC, "msm.hip"), "-o", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    with open(out) as f:
        blocks = _blocks(f.read())
    # the blocks of field products; the canonical-form code of the exceptional case has hundreds of multiply-adds too, but also
    # hundreds of moves, and is not part of the addition's path
    prod = [i for i, b in enumerate(blocks) if b.ops()["v_mad_u64_u32"] >= 100 and len(b.moves()) <= 16]
    # the loop: the blocks on a cycle through the first block of products
    body = {i for i in _reach(blocks, prod[0]) if prod[0] in _reach(blocks, i)}
    prod = [i for i in prod if i in body]
    assert sum(blocks[i].ops()["v_mad_u64_u32"] for i in prod) == 1467, [blocks[i].label for i in prod]
    gather = [i for i in body if blocks[i].ops()["global_load_dwordx4"]]
    assert len(gather) == 1, [blocks[i].label for i in gather]
    preds = collections.defaultdict(set)
    for i, b in enumerate(blocks):
        for s in b.succ:
            preds[s].add(i)
    heads = [i for i in body if preds[i] - body]
    assert len(heads) == 1, [blocks[i].label for i in heads]
    head, need = heads[0], set(prod) | set(gather)
    best = [None]

    def walk(node, path, seen):
        for s in blocks[node].succ:
            if s == head:
                if need <= seen:
                    cost = sum(blocks[i].valu() for i in path)
                    if best[0] is None or cost < best[0][0]:
                        best[0] = (cost, list(path))
            elif s in body and s not in seen:
                path.append(s)
                seen.add(s)
                walk(s, path, seen)
                seen.discard(s)
                path.pop()

    walk(head, [head], {head})
    assert best[0], "no way round the loop through the products and the row gather"
    return {"blocks": blocks, "body": body, "path": best[0][1], "prod": prod, "gather": gather[0], "preds": preds}


def _regs(operand):
    m = re.match(r"v\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", operand)
    return {int(m.group(1))} if m else set()


def test_no_copies_of_row_or_accumulator_at_the_loop_end(loop):
    blocks, path = loop["blocks"], loop["path"]
    outside = [i for i in path if i not in loop["prod"]]
    row = set()
    for ins in blocks[loop["gather"]].ins:
        if ins.startswith("global_load_dwordx4"):
            row |= _regs(ins.split()[1].rstrip(","))
    assert len(row) == 16, sorted(row)  # four 16-byte loads, nothing overlapping
    assert blocks[loop["gather"]].ops()["global_load_dwordx4"] == 4
    moves = [m for i in outside for m in blocks[i].moves()]
    for m in moves:
        dst, src = [x.rstrip(",") for x in m.split()[1:3]]
        assert not (_regs(dst) | _regs(src)) & row, m
    # what is left are loop counters and the sign of the next entry: 36 accumulator limbs cannot hide in this
    assert len(moves) <= 6, moves
    latch = [i for i in path if loop["path"][0] in blocks[i].succ]
    assert len(latch) == 1 and len(blocks[latch[0]].moves()) <= 4, [blocks[i].moves() for i in latch]


def test_no_one_constants_on_the_steady_path(loop):
    blocks = loop["blocks"]
    for i in loop["path"]:
        for ins in blocks[i].ins:
            for k in ONE:
                assert ("0x%x" % k) not in ins.lower() and (" %d" % k) not in ins, (blocks[i].label, ins)
    # they do exist in the loop, on the run-start path
    assert any(("0x%x" % ONE[0]) in ins.lower() for i in loop["body"] for ins in blocks[i].ins)


def test_run_end_path_does_not_drain_the_row_prefetch(loop):
    blocks, body, steady = loop["blocks"], loop["body"], set(loop["path"])
    stores = [i for i in body if any(x.startswith("global_store") for x in blocks[i].ins)]
    assert stores and not set(stores) & steady
    region = set(stores)
    for i in stores:  # the blocks between the steady path and the partial's store, both ways
        region |= _reach(blocks, i, body - steady)
        todo = [i]
        while todo:
            for q in loop["preds"][todo.pop()]:
                if q in body and q not in steady and q not in region:
                    region.add(q)
                    todo.append(q)
    for i in region:
        for ins in blocks[i].ins:
            assert not (ins.startswith("s_waitcnt") and "vmcnt(0)" in ins), (blocks[i].label, ins)
        # one load at most (the end of the run after the next), none that depends on another
        assert blocks[i].ops()["global_load_dword"] <= 1, blocks[i].label


def test_vector_instructions_around_the_products(loop):
    blocks, path = loop["blocks"], loop["path"]
    outside = sum(blocks[i].valu() for i in path if i not in loop["prod"])
    total = sum(blocks[i].valu() for i in path)
    print("steady path:", [(blocks[i].label, blocks[i].valu()) for i in path], "outside the products:", outside, "total:", total)
    assert outside <= OUTSIDE_VALU_MAX, outside
    assert total <= PATH_VALU_MAX, total
