"""CPU: what tests/test_gpu_step_waits.py relies on and what csrc/step.hip's hand-counted waits rely on.

 a. tests/step_report.py - the arithmetic that places a bad output element in the kernel (block, tile within the
    block, lane, worker, slot): synthetic bad masks in, the expected places out; the slot map restated there puts
    every field and the dense pseudo-field into exactly one (worker, slot).
 b. the emitted code against the declared sequence.  csrc/step.hip derives its `s_waitcnt vmcnt(N)` counts for one
    fixed sequence of vector-memory operations per segment and says "checked against the emitted order" - here that
    check is a test: step.hip is compiled to gfx950 assembly text (skipped without hipcc) and, for each of the six
    instantiations of deepfm_step_kernel, the two tile loops (a label with a backward branch to it around an
    s_barrier: exactly two, or the test FAILS) must hold the declared operations in the declared order, no scratch
    access, no other wait on vmcnt than the declared ones, and - replayed as an in-order queue over three iterations -
    every wait must retire exactly the operation its derivation awaits, no fewer and no more; no instruction between
    an entry load and its wait may name the load's destination register.
    The checker itself is tested on assembly text generated from the declared sequence and on altered copies of it
    (and of the compiler's text): a count changed, an operation removed, a register named early, ... must each fail.
"""
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import step_report as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = os.path.join(ROOT, "recman_amd", "csrc", "step.hip")


# ------------------------------------------------------------------------------------------- a. the failure report
def test_report_arithmetic_is_the_kernels():
    RP.cite_all()


@pytest.mark.parametrize("F,Dn", [(F, Dn) for F in range(1, 27) for Dn in (0, 13)])
def test_slot_map_puts_every_field_into_exactly_one_worker_and_slot(F, Dn):
    at = RP.slot_map(F, Dn)
    assert sorted(at) == list(range(F + (1 if Dn else 0)))
    assert len(set(at.values())) == len(at) and all(0 <= w < 7 and 0 <= j < 4 for w, j in at.values())
    assert (3, 3) not in at.values()                      # the head's SIMD partner sits out the last round
    for f, (w, j) in at.items():
        assert RP.slot_field(w, j) == f
    hits = {f: sum(RP.slot_field(w, j) == f for w in range(7) for j in range(4)) for f in at}
    assert set(hits.values()) == {1}


def _image_read(w, j, F, Dn):
    """The LDS image slot j of worker w reads (slot_base in csrc/step.hip, restated): a field's ring buffers, the
    dense ring or the zero image."""
    RP._cite("return __builtin_amdgcn_readfirstlane(sx[j] ? ring : (sv[j] ? dn : oZero));")
    RP._cite("sv[j] = f >= 0 && (f < F || (f == F && a.Dn > 0));")
    RP._cite("sx[j] = f >= 0 && f < F;")
    RP._cite("fld[j] = sv[j] ? f : 0;")
    f = RP.slot_field(w, j)
    sv, sx = f >= 0 and (f < F or (f == F and Dn > 0)), 0 <= f < F
    return ("ring", f if sv else 0) if sx else (("dense",) if sv else ("zero",))


@pytest.mark.parametrize("F,Dn", [(F, Dn) for F in range(1, 27) for Dn in (0, 13)])
def test_a_ring_buffer_is_read_by_the_worker_that_fetches_it_alone(F, Dn):
    """A row DMA is covered by the issuing wave's counted wait and by nothing else (the tile barrier does not wait
    for vector memory), so no other wave may read what it fetches - empty slots included: they once ran on field
    0's buffer with zero weights, and zero times the NaN bits of a buffer not yet written is NaN."""
    at = RP.slot_map(F, Dn)
    for w in range(7):
        for j in range(4):
            img = _image_read(w, j, F, Dn)
            if img[0] == "ring":
                assert at[img[1]] == (w, j), f"worker {w} slot {j} reads field {img[1]}'s rows, worker {at[img[1]][0]}'s DMA"
            elif img[0] == "dense":
                assert Dn > 0 and at[F] == (w, j)
            else:
                assert RP.slot_field(w, j) not in at
    assert _image_read(3, 3, F, Dn) == ("zero",)


def test_examples_are_placed_by_the_launch_arithmetic():
    B = 16 * 256 * 3 + 5                                   # 769 tiles on 256 blocks: block 0 runs 4, the others 3
    assert RP.launch(B) == (769, 256)
    assert RP.locate(0, B) == (0, 0, 0, True)
    assert RP.locate(16 * 256 + 3, B) == (0, 1, 3, True)           # tile 256 = block 0's second
    assert RP.locate(16 * (256 * 2 + 255) + 15, B) == (255, 2, 15, True)
    assert RP.locate(B - 1, B) == (0, 3, 4, False)                 # the ragged tile: block 0's fourth, past the fill
    assert RP.locate(79, 80) == (4, 0, 15, True)                   # five blocks of one tile
    # every example once, and tile counts as the kernel's T
    for B in (80, 16 * 775, 12293):
        ntiles, nblk = RP.launch(B)
        seen = {}
        for b in range(B):
            blk, tile, n, fill = RP.locate(b, B)
            assert fill == (tile < 3) and 0 <= n < 16 and (blk + tile * nblk) * 16 + n == b
            seen[blk] = max(seen.get(blk, 0), tile + 1)
        assert [seen[k] for k in range(nblk)] == [-(-(ntiles - k) // nblk) for k in range(nblk)]


def test_synthetic_bad_masks_come_out_at_the_expected_places():
    B, F, Dn = 16 * 256 * 3 + 5, 26, 13
    # per-example outputs
    m = torch.zeros(B, dtype=torch.bool)
    m[[5, 16 * 256 + 3, B - 1]] = True
    got = RP.describe("logit", m, B, F, Dn, values=[torch.arange(B).float()])
    assert got[0] == f"logit: 3 of {B} elements"
    assert got[1] == "  b 5 = block 0 tile 0 (fill: first three) lane n 5 [5]"
    assert got[2] == "  b 4099 = block 0 tile 1 (fill: first three) lane n 3 [4099]"
    assert got[3] == f"  b {B - 1} = block 0 tile 3 (steady) lane n 4 [{B - 1}]"
    # ... capped at 32 and counted
    got = RP.describe("pred", torch.ones(B, dtype=torch.bool), B, F, Dn)
    assert len(got) == 1 + 32 + 1 and got[-1] == f"  ... and {B - 32} more examples"
    # row gradients: fields -> (worker, slot)
    m = torch.zeros(B, F, 16, dtype=torch.bool)
    m[16 * 300 + 2, 3, 7] = m[16 * 300 + 2, 24, 0] = m[40, 10, 15] = True
    got = RP.describe("d_rows", m, B, F, Dn)
    assert got[1] == "  fields 3 (worker 3 slot 0), 10 (worker 3 slot 1), 24 (worker 4 slot 3)"
    assert got[2] == "  b 40 = block 2 tile 0 (fill: first three) lane n 8 fields [10]"
    assert got[3] == "  b 4802 = block 44 tile 1 (fill: first three) lane n 2 fields [3, 24]"
    # the packed form: a row of the send buffer is the occurrence that addresses it
    pos = torch.arange(B * F).reshape(B, F) * 2 + 1
    m = torch.zeros(2 * B * F + 2, 20, dtype=torch.bool)
    m[int(pos[4802, 21]), 17] = True
    m[0, 0] = True                                          # a row nobody addresses
    got = RP.describe("d_rows", m, B, F, Dn, pos=pos, values=[torch.full(m.shape, 2.5)])
    assert got[1] == "  1 rows of the send buffer that no occurrence addresses, first [0]"
    assert got[2] == "  fields 21 (worker 0 slot 3)"
    assert got[3] == "  b 4802 = block 44 tile 1 (fill: first three) lane n 2 fields [21] [2.5]"
    # dW0: row ranges are fields, the rows past 16 F the dense pseudo-field (F = 26: worker 6's last slot)
    m = torch.zeros(16 * F + Dn, 32, dtype=torch.bool)
    m[16 * 7: 16 * 8] = True
    m[16 * F + 2, 5] = True
    got = RP.describe("dW0", m, B, F, Dn)
    assert got[1] == "  rows 112..127 (16 of them): field 7 (worker 0 slot 1)"
    assert got[2] == "  rows 418..418 (1 of them): the dense pseudo-field (worker 6 slot 3)"
    # the head's sums
    got = RP.describe("db1", torch.tensor([False, True] * 16), B, F, Dn, values=[torch.zeros(32), torch.ones(32)])
    assert got[0] == "db1: 16 of 32 elements" and "[1, 3, 5" in got[1] and "[0 / 1]" in got[1]
    assert RP.describe("loss", torch.zeros(1, dtype=torch.bool), B, F, Dn) == []


def test_findings_collect_every_output_before_raising():
    B, F, Dn = 80, 7, 0
    fnd = RP.Findings("case", B, F, Dn)
    fnd.raise_if_any()
    nan = torch.zeros(B)
    nan[17] = float("nan")
    fnd.add("NaN", "logit", ~torch.isfinite(nan), values=[nan])
    fnd.add("NaN", "dlogit", torch.zeros(B, dtype=torch.bool))
    fnd.add("NaN", "dW0", torch.ones(16 * F, 32, dtype=torch.bool))
    with pytest.raises(AssertionError) as e:
        fnd.raise_if_any()
    text = str(e.value)
    assert "case: B 80 F 7 Dn 0: 5 tiles on 5 blocks" in text
    assert "[NaN] logit: 1 of 80" in text and "b 17 = block 1 tile 0 (fill: first three) lane n 1 [nan]" in text
    assert "dlogit" not in text and "[NaN] dW0" in text and "field 6 (worker 6 slot 0)" in text


def test_tolerance_masks_restate_the_kernel_tests_tolerances():
    want = dict(logit=torch.tensor([1.0, -2.0]).double(), loss=torch.tensor([0.7]).double(),
                d_rows=torch.tensor([[[1.0] * 16, [1e-3] * 16]]).double(), dW0=None)
    got = dict(logit=torch.tensor([1.0 + 9e-6, -2.0 + 1.2e-5]), loss=torch.tensor([0.7 + 5e-6]),
               d_rows=torch.tensor([[[1.0 + 1e-5] * 16, [1e-3 + 3e-6] * 16]]), dW0=torch.zeros(2))
    m = RP.tolerance_masks(got, want)
    assert m["logit"].tolist() == [False, True] and m["loss"].tolist() == [False] and "dW0" not in m
    assert not m["d_rows"][0, 0].any() and m["d_rows"][0, 1].all()      # 3e-6 > 2e-5 * max(1e-3, 0.1)
    got["logit"][0] = float("nan")
    assert RP.tolerance_masks(got, want)["logit"].tolist() == [True, True]


# --------------------------------------------------------------------------- b. the emitted code, declared sequence
VM_PREFIXES = ("global_load", "global_store", "buffer_load", "buffer_store", "flat_", "scratch_")
KERNEL = re.compile(r"^(_ZN\S*deepfm_step_kernelILb([01])ELb([01])ELb([01])E\w*):")
INSTANCES = {(1, 0, 1), (0, 0, 1), (1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0)}  # <NT, NT_OUT, PACKED>, as launched
HEAD_WAITS = (10, 3)   # wait A: the label's load, wait B: the last id's (derived in step_head)


def _declared():
    """The constants as csrc/step.hip derives them; the text is cited so that a new derivation is restated here."""
    with open(STEP) as f:
        src = " ".join(f.read().split())
    for text in ("constexpr int kSP = PACKED ? 2 : 1;",
                 "constexpr int kYoungerE = 7 + 4 * kSP, kYounger = 8 + 6 * kSP;",
                 "E_0 D_0 | E_1 D_1 S_0 | E_2 D_2 S_1 | E_3 D_3 S_2 | S_3 = 8 + 4 SP operations per segment",
                 "St St St | [wait A: dense + label] [wait B: ids] | Dn Dn Dn Dn Y | Id x 7 = 15 operations per segment",
                 'asm volatile("s_waitcnt vmcnt(10)" : "+v"(dnr[0])', 'asm volatile("s_waitcnt vmcnt(3)" : "+v"(idr[0])'):
        assert text in src.replace("// ", ""), f"csrc/step.hip no longer says `{text}`: re-derive the counts here"
    for a in sorted(INSTANCES):
        assert "RM_STEP({}, {}, {})".format(*("true" if x else "false" for x in a)) in src


def worker_sequence(sp):
    return ["E", "D"] + (["E", "D"] + ["S"] * sp) * 3 + ["S"] * sp


def head_sequence():
    return ["S"] * 3 + ["E"] * 12


def _kernels(text):
    """{(NT, NT_OUT, PACKED): [instruction lines]} of every deepfm_step_kernel in the assembly text; a line is
    (mnemonic or label, operand text) with comments and directives dropped."""
    out, cur = {}, None
    for raw in text.splitlines():
        m = KERNEL.match(raw)
        if m:
            cur = tuple(int(x) for x in m.groups()[1:])
            assert cur not in out, f"instantiation {cur} twice"
            out[cur] = []
            continue
        if cur is None:
            continue
        line = raw.split(";")[0].strip()
        if line.startswith(".Lfunc_end"):
            cur = None
        elif re.match(r"^\.LBB\d+_\d+:$", line):
            out[cur].append((line[:-1], ""))
        elif line and not line.startswith("."):
            op, _, rest = line.partition(" ")
            op, _, rest2 = op.partition("\t")
            out[cur].append((op, (rest2 + " " + rest).strip()))
    return out


def _tile_loops(lines):
    """[(first, last)] line ranges of the loops - a label and the furthest backward branch to it that control can
    reach from the label - that hold an s_barrier."""
    at = {op: i for i, (op, _) in enumerate(lines) if op.startswith(".LBB")}
    back = {}
    for i, (op, rest) in enumerate(lines):
        if op == "s_branch" or op.startswith("s_cbranch"):
            tgt = rest.strip()
            assert tgt in at, f"branch to an unknown label {tgt}"
            if at[tgt] < i:
                back[at[tgt]] = i

    def reaches(a, b):  # control flows from line a to line b (a block laid out behind its successor is no loop)
        seen, todo = set(), [a]
        while todo:
            i = todo.pop()
            if i == b:
                return True
            if i in seen or i >= len(lines):
                continue
            seen.add(i)
            op, rest = lines[i]
            if op == "s_branch" or op.startswith("s_cbranch"):
                todo.append(at[rest.strip()])
            if op not in ("s_branch", "s_endpgm"):
                todo.append(i + 1)
        return False

    loops = [(a, b) for a, b in sorted(back.items())
             if any(op == "s_barrier" for op, _ in lines[a:b]) and reaches(a, b)]
    for (a0, b0), (a1, b1) in zip(loops, loops[1:]):
        assert b0 < a1, "tile loops overlap"
    return loops


def _regs(rest):
    """The VGPR numbers an operand text names."""
    r = {int(x) for x in re.findall(r"(?<![\w\[])v(\d+)\b", rest)}
    for a, b in re.findall(r"(?<!\w)v\[(\d+):(\d+)\]", rest):
        r |= set(range(int(a), int(b) + 1))
    return r


def _events(body, what):
    """The loop body's vector-memory operations and vmcnt waits in emitted order: (line, 'E' | 'D' | 'S' | 'W', count)."""
    ev = []
    for i, (op, rest) in enumerate(body):
        if op.startswith(VM_PREFIXES):
            assert not op.startswith("scratch_"), f"{what}: a scratch access in the tile loop: {op} {rest}"
            if op == "global_load_dword":
                ev.append((i, "E", None))
            elif op == "global_load_lds_dwordx4":
                ev.append((i, "D", None))
            elif op in ("buffer_store_dword", "buffer_store_dwordx4"):
                ev.append((i, "S", None))
            else:
                raise AssertionError(f"{what}: a vector-memory operation the declared sequence does not have: {op} {rest}")
        elif op == "s_waitcnt" and "vmcnt" in rest:
            ev.append((i, "W", int(re.search(r"vmcnt\((\d+)\)", rest).group(1))))
    return ev


def _check_loop(body, what, sequence, waits):
    """waits: [(count, ordinal of the 'E' / 'D' operation of the PREVIOUS iteration it awaits as (kind, k), number of
    this iteration's operations issued in front of it)] in emitted order."""
    ev = _events(body, what)
    ops = [e for e in ev if e[1] != "W"]
    kinds = [k for _, k, _ in ops]
    assert len(kinds) == len(sequence), f"{what}: {len(kinds)} vector-memory operations, declared {len(sequence)}: {kinds}"
    assert kinds == sequence, f"{what}: emitted order {kinds}, declared {sequence}"
    got = [c for _, k, c in ev if k == "W"]
    assert 0 not in got, f"{what}: s_waitcnt vmcnt(0) in the tile loop"
    assert got == [w[0] for w in waits], f"{what}: waits on vmcnt {got}, declared {[w[0] for w in waits]}"
    # ---- replay: an in-order queue, three iterations; the waits of iterations 1 and 2 are checked
    ordinal, seen = [], {}
    for _, k, _ in ops:
        ordinal.append((k, seen.get(k, 0)))
        seen[k] = seen.get(k, 0) + 1
    issued = []
    for it in range(3):
        wi = 0
        n_here = 0
        for _, k, count in ev:
            if k != "W":
                issued.append((it,) + ordinal[n_here])
                n_here += 1
                continue
            _, awaited, in_front = waits[wi]
            wi += 1
            assert n_here == in_front, f"{what}: wait {wi} stands behind {n_here} operations of its segment, declared {in_front}"
            if it == 0:
                continue
            youngest_retired = len(issued) - count - 1
            want = issued.index((it - 1,) + awaited)
            assert youngest_retired >= want, \
                f"{what}: vmcnt({count}) leaves {awaited[0]}_{awaited[1]} of the previous segment in flight " \
                f"({want - youngest_retired} too large)"
            assert youngest_retired == want, \
                f"{what}: vmcnt({count}) retires {youngest_retired - want} operations more than the derivation says"
    # ---- no instruction between an entry load and the wait in front of its use names its destination register
    wait_lines = [i for i, k, _ in ev if k == "W"]
    for (line, k, _), (_, o) in zip(ops, ordinal):
        if k != "E":
            continue
        mine = [wl for wl, w in zip(wait_lines, waits) if w[1][0] == "E" and w[1][1] >= o][0]
        dst = _regs(body[line][1].split(",")[0])
        assert len(dst) == 1, f"{what}: destination of {body[line]}"
        assert mine < line, f"{what}: the wait of E_{o} does not stand in front of its reload"
        for op, rest in body[line + 1:] + body[:mine]:
            assert not (dst & _regs(rest)), \
                f"{what}: `{op} {rest}` names v{min(dst)} between its load (E_{o}) and the wait in front of its use"


def _worker_counts(sp):
    return 7 + 4 * sp, 8 + 6 * sp   # kYoungerE, kYounger as csrc/step.hip derives them (cited in _declared)


def check_step_asm(text, worker_counts=_worker_counts, head_waits=HEAD_WAITS):
    """Every assertion of section b on the assembly text of csrc/step.hip.  (The counts are arguments so that the
    replay can be shown to refuse a wrong DERIVATION - code and declaration agreeing on a count that is off by one.)"""
    kernels = _kernels(text)
    assert set(kernels) == INSTANCES, f"instantiations found: {sorted(kernels)}"
    for inst, lines in sorted(kernels.items()):
        sp = 2 if inst[2] else 1
        loops = _tile_loops(lines)
        assert len(loops) == 2, f"{inst}: {len(loops)} tile loops (a label, a backward branch to it, an s_barrier inside), not 2"
        bodies = [lines[a:b + 1] for a, b in loops]
        dma = [any(op.startswith("global_load_lds") for op, _ in b) for b in bodies]
        assert sorted(dma) == [False, True], f"{inst}: one tile loop with LDS-DMAs (the workers') and one without (the head's)"
        worker, head = (bodies[0], bodies[1]) if dma[0] else (bodies[1], bodies[0])
        ke, ky = worker_counts(sp)
        _check_loop(worker, f"{inst} workers", worker_sequence(sp),
                    [(ke, ("E", 0), 0), (ke, ("E", 1), 2), (ke, ("E", 2), 4 + sp), (ke, ("E", 3), 6 + 2 * sp),
                     (ky, ("D", 3), 8 + 4 * sp)])
        _check_loop(head, f"{inst} head", head_sequence(),
                    [(head_waits[0], ("E", 4), 3), (head_waits[1], ("E", 11), 3)])


# ---- the checker on text generated from the declared sequence, and on altered copies of it
def _synthetic_kernel(k, inst):
    sp = 2 if inst[2] else 1
    ke, ky = 7 + 4 * sp, 8 + 6 * sp
    name = "_ZN12_GLOBAL__N_118deepfm_step_kernelILb{}ELb{}ELb{}EEEvNS_8StepArgsE".format(*inst)
    t = [f"{name}: ; @{name}", "\ts_load_dwordx4 s[0:3], s[4:5], 0x0", f"\ts_cbranch_scc0 .LBB{k}_9"]
    # the head's loop, its first segment peeled in front of it as hipcc does
    head = ["\tbuffer_store_dword v4, v191, s[4:7], 0 offen"] * 3 + \
           ["\ts_waitcnt vmcnt(10)", "\tds_write_b128 v1, v[197:200]", "\ts_waitcnt vmcnt(3)", "\tds_write_b32 v1, v201"] + \
           [f"\tglobal_load_dword v{197 + i}, v[6:7], off" for i in range(12)] + ["\ts_waitcnt lgkmcnt(0)", "\ts_barrier"]
    t += head + [f".LBB{k}_1: ; =>This Inner Loop Header: Depth=1", "\tv_mfma_f32_16x16x4_f32 v[0:3], v8, v9, v[0:3]"] + head
    t += [f"\ts_cbranch_scc1 .LBB{k}_2", f"\ts_branch .LBB{k}_1", f".LBB{k}_2:", "\ts_waitcnt vmcnt(0)",
          "\tglobal_store_dword v[20:21], v10, off", "\ts_endpgm", f".LBB{k}_9:"]
    # the workers' loop
    t += [f".LBB{k}_10: ; =>This Inner Loop Header: Depth=1", "\tds_read_b128 v[10:13], v5"]
    store = ["\tbuffer_store_dwordx4 v[10:13], v112, s[88:91], 0 offen"] * sp
    for j in range(4):
        t += [f"\ts_waitcnt vmcnt({ke})", f"\tv_add_f32 v120, v120, v{113 + j}",
              f"\tglobal_load_dword v{113 + j}, v[66:67], off", "\tglobal_load_lds_dwordx4 v[62:63], off",
              "\tv_mfma_f32_16x16x4_f32 v[0:3], v8, v9, v[0:3]"] + (store if j else [])
    t += store + [f"\ts_cbranch_vccnz .LBB{k}_11", f"\ts_waitcnt vmcnt({ky})", "\tds_read_b128 v[14:17], v5",
                  f".LBB{k}_11:", "\ts_waitcnt lgkmcnt(0)", "\ts_barrier", f"\ts_cbranch_scc1 .LBB{k}_12",
                  f"\ts_branch .LBB{k}_10", f".LBB{k}_12:", "\ts_waitcnt vmcnt(0)", "\ts_endpgm", f".Lfunc_end{k}:"]
    return t


def _synthetic():
    return "\n".join(l for k, inst in enumerate(sorted(INSTANCES)) for l in _synthetic_kernel(k, inst))


def _alter(text, old, new, nth=0, after=""):
    """text with the nth occurrence of the line `old` behind the first line containing `after` replaced by `new`
    (None: removed)."""
    lines = text.splitlines()
    start = next(i for i, l in enumerate(lines) if after in l)
    hits = [i for i in range(start, len(lines)) if lines[i].strip() == old]
    i = hits[nth]
    lines[i: i + 1] = [] if new is None else ["\t" + new]
    return "\n".join(lines)


ALTERED = [
    ("a worker count one too large", "s_waitcnt vmcnt(11)", "s_waitcnt vmcnt(12)", 2, "declared [11, 11, 11, 11, 14]"),
    ("a worker count one too small", "s_waitcnt vmcnt(11)", "s_waitcnt vmcnt(10)", 1, "declared [11, 11, 11, 11, 14]"),
    ("the forward's count too large", "s_waitcnt vmcnt(14)", "s_waitcnt vmcnt(15)", 0, "declared [11, 11, 11, 11, 14]"),
    ("the packed forward's count too small", "s_waitcnt vmcnt(20)", "s_waitcnt vmcnt(19)", 0, "declared [15, 15, 15, 15, 20]"),
    ("a store removed", "buffer_store_dwordx4 v[10:13], v112, s[88:91], 0 offen", None, 0, "vector-memory operations, declared"),
    ("a DMA removed", "global_load_lds_dwordx4 v[62:63], off", None, 0, "vector-memory operations, declared"),
    ("a store moved in front of the first pair", "ds_read_b128 v[10:13], v5",
     "buffer_store_dwordx4 v[10:13], v112, s[88:91], 0 offen", 0, "vector-memory operations, declared"),
    ("the head's wait A too large", "s_waitcnt vmcnt(10)", "s_waitcnt vmcnt(11)", 1, "declared"),
    ("a full drain in the loop", "ds_read_b128 v[10:13], v5", "s_waitcnt vmcnt(0)", 0, "vmcnt(0) in the tile loop"),
    ("a scratch reload in the loop", "ds_read_b128 v[10:13], v5", "scratch_load_dword v113, off, s0", 0, "scratch access"),
    ("another kind of load", "global_load_dword v114, v[66:67], off", "global_load_dwordx2 v[114:115], v[66:67], off", 0,
     "the declared sequence does not have"),
    ("an entry register copied before its wait", "ds_read_b128 v[14:17], v5", "v_mov_b32 v30, v115", 0, "names v115"),
    ("an entry register inside a register range", "ds_read_b128 v[14:17], v5", "ds_write_b128 v5, v[113:116]", 0, "names v113"),
    ("a prefetch register read early", "v_mfma_f32_16x16x4_f32 v[0:3], v8, v9, v[0:3]", "v_cvt_f32_i32 v30, v201", 0, "names v201"),
    ("no barrier in the head's loop", "s_barrier", "s_nop 0", 1, "tile loops"),
]


def test_the_checker_passes_the_declared_sequence():
    _declared()
    check_step_asm(_synthetic())


@pytest.mark.parametrize("what,old,new,nth,message", ALTERED, ids=[a[0] for a in ALTERED])
def test_the_checker_fails_an_altered_copy(what, old, new, nth, message):
    text = _alter(_synthetic(), old, new, nth)
    assert text != _synthetic()
    with pytest.raises(AssertionError, match=re.escape(message)):
        check_step_asm(text)


@pytest.mark.parametrize("de,dy,da,db,message", [
    (1, 0, 0, 0, "leaves E_0 of the previous segment in flight (1 too large)"),
    (-1, 0, 0, 0, "retires 1 operations more than the derivation says"),
    (0, 1, 0, 0, "leaves D_3 of the previous segment in flight (1 too large)"),
    (0, -2, 0, 0, "retires 2 operations more than the derivation says"),
    (0, 0, 1, 0, "leaves E_4 of the previous segment in flight (1 too large)"),
    (0, 0, 0, -1, "retires 1 operations more than the derivation says")])
def test_the_replay_refuses_a_derivation_that_is_off_in_either_direction(de, dy, da, db, message):
    """Code and declaration agree on a count, and the count is wrong: only the replay of the queue can tell."""
    text = _synthetic()
    for sp in (1, 2):
        ke, ky = _worker_counts(sp)
        text = text.replace(f"vmcnt({ke})", f"vmcnt(#{ke + de})").replace(f"vmcnt({ky})", f"vmcnt(#{ky + dy})")
    text = text.replace("vmcnt(10)", f"vmcnt(#{10 + da})").replace("vmcnt(3)", f"vmcnt(#{3 + db})").replace("#", "")
    with pytest.raises(AssertionError, match=re.escape(message)):
        check_step_asm(text, lambda sp: (_worker_counts(sp)[0] + de, _worker_counts(sp)[1] + dy), (10 + da, 3 + db))


def test_the_checker_reads_registers_and_loops():
    assert _regs("v113, v[66:67], off") == {113, 66, 67} and _regs("v[10:13], s[88:91], 0 offen") == {10, 11, 12, 13}
    assert _regs("s113, a113, 0x113") == set()
    k = _kernels(_synthetic())
    assert set(k) == INSTANCES and all(len(_tile_loops(v)) == 2 for v in k.values())
    with pytest.raises(AssertionError, match="instantiations found"):
        check_step_asm("\n".join(_synthetic_kernel(0, (0, 0, 0))))
    with pytest.raises(AssertionError, match="instantiations found"):
        check_step_asm("")


@pytest.fixture(scope="module")
def step_asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found: csrc/step.hip cannot be compiled to assembly text here")
    from recman_amd import build
    out = str(tmp_path_factory.mktemp("step_asm") / "step.s")
    # recman_amd/build.py's flags, -S instead of -c, the device side alone
    cmd = [hipcc, "-O3", "-std=c++17", f"--offload-arch={build.ARCH}", "-fPIC", "-S", "--cuda-device-only", STEP,
           "-o", out, "-Wall", "-Wno-unused-function"]
    subprocess.run(cmd, check=True, capture_output=True)
    with open(out) as f:
        return f.read()


def test_emitted_tile_loops_hold_the_declared_sequence_and_waits(step_asm):
    _declared()
    check_step_asm(step_asm)


def test_the_checker_fails_an_altered_copy_of_the_emitted_code(step_asm):
    plain = "deepfm_step_kernelILb0ELb0ELb0E"
    for old, new, nth, message in [
            ("s_waitcnt vmcnt(11)", "s_waitcnt vmcnt(12)", -1, "declared"),             # the loop's last entry wait
            ("s_waitcnt vmcnt(14)", "s_waitcnt vmcnt(13)", -1, "declared"),
            ("s_waitcnt vmcnt(3)", "s_waitcnt vmcnt(4)", -1, "declared"),
            ("s_barrier", None, -1, "tile loops")]:
        lines = step_asm.splitlines()
        start = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and plain in l)
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        hits = [i for i in range(start, end) if lines[i].split(";")[0].strip() == old]
        lines[hits[nth]: hits[nth] + 1] = [] if new is None else ["\t" + new]
        with pytest.raises(AssertionError, match=re.escape(message)):
            check_step_asm("\n".join(lines))
    # an operation removed: the last d_rows store of the plain kernel's worker loop
    lines = step_asm.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and plain in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    last = [i for i in range(start, end) if lines[i].strip().startswith("buffer_store_dwordx4")][-1]
    del lines[last]
    with pytest.raises(AssertionError, match="vector-memory operations, declared"):
        check_step_asm("\n".join(lines))
