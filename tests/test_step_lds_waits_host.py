"""CPU: the workers' counted LDS waits of csrc/step.hip, checked in the emitted code.

In front of each row DMA D_j (global_load_lds_dwordx4) of the worker loop stands an `s_waitcnt lgkmcnt(N)` that must
have brought back this wave's reads of the ring image the DMA overwrites - and should leave the later slots' reads in
flight, under the matrix work.  A GPU run cannot catch a count that is too weak: the DMA's data lands hundreds of
cycles after the reads have returned anyway.  So, as tests/test_step_waits_host.py does for vmcnt, step.hip is
compiled to gfx950 assembly text (skipped without hipcc) and for each of the six instantiations one iteration of the
worker loop is walked along the path that runs a backward, a DMA and a forward, with the LDS counter replayed as the
in-order queue it is:

 * the R phase is the R reads the source declares (28, PACKED 32), every one in front of the first DMA, and no other
   LDS operation and no scalar memory read (they share the counter and return out of order) stands between the loop
   top and D_3;
 * at D_k the first R_k = R - 3 (3 - k) reads have returned - no fewer (the image is still being read) and no more
   (the wait would be a drain again);
 * the waits on lgkmcnt from the loop top to D_3 are tile_barrier's and the four derived ones, 9 6 3 0, each between
   D_(k-1) and D_k.  The last count is 0 by derivation (slot 3 is read last), not a drain in front of the matrix work:
   three MFMA groups (48) stand in front of it.  No other lgkmcnt(0) may stand there;
 * hipcc does not count the asm reads, so no instruction between a read and the wait that covers it may name the
   read's destination registers;
 * no scratch access in the loop.

The checker is shown to fail on altered copies of the emitted code: a count raised by one, a count lowered by one, a
read moved behind its wait's DMA, a destination register named early, a drain, a scratch access.
"""
import re

import pytest

from tests.test_step_waits_host import INSTANCES, STEP, _kernels, _regs, _tile_loops, step_asm  # noqa: F401 (fixture)

SLOT_READS = 3          # 2 x ds_read2st64_b32 (columns) + ds_read_b128 (e4)
SMEM = re.compile(r"^s_(load|memtime|memrealtime)")


def _declared(packed):
    """R and the counts as csrc/step.hip derives them; the text is cited so that a new derivation is restated here."""
    with open(STEP) as f:
        src = " ".join(f.read().replace("//", " ").split())
    for text in ("slot j = 0, 1, 2, 3: columns of examples q, 4 + q and 8 + q, 12 + q (2 x ds_read2st64_b32), e4 (b128) 3 each",
                 "s_waitcnt lgkmcnt(3 (3 - j)) = 9, 6, 3, 0 behind slot j's last read: the 3 reads of each slot j + 1 .. 3",
                 "of the R = 28 (PACKED 32) reads of the segment the first R_j = R - 3 (3 - j) have returned at D_j",
                 'if (j == 1) asm volatile("s_waitcnt lgkmcnt(6)" : RM_SLOT_REGS(r)::"memory");',
                 'else if (j == 2) asm volatile("s_waitcnt lgkmcnt(3)" : RM_SLOT_REGS(r)::"memory");',
                 'else asm volatile("s_waitcnt lgkmcnt(0)" : RM_SLOT_REGS(r)::"memory");'):
        assert text in src, f"csrc/step.hip no longer says `{text}`: re-derive the counts here"
    assert src.count('asm volatile("s_waitcnt lgkmcnt(9)"') == 2     # slot_wait0, plain and PACKED
    R = 32 if packed else 28
    return R, [R - SLOT_READS * (3 - k) for k in range(4)], [SLOT_READS * (3 - k) for k in range(4)]


def _worker_loop(lines, what):
    loops = _tile_loops(lines)
    assert len(loops) == 2, f"{what}: {len(loops)} tile loops, not 2"
    bodies = [lines[a:b + 1] for a, b in loops if any(op.startswith("global_load_lds") for op, _ in lines[a:b + 1])]
    assert len(bodies) == 1, f"{what}: {len(bodies)} tile loops with LDS-DMAs"
    return bodies[0]


def _iteration(body, what):
    """One iteration in execution order along the path that does everything: conditional branches fall through (they
    skip the MFMAs of a segment without a backward, the forward, or leave the loop), unconditional ones are followed;
    the walk ends at the branch back to the loop's label."""
    top = body[0][0]
    assert top.startswith(".LBB"), f"{what}: the loop does not start at a label"
    at = {op: i for i, (op, _) in enumerate(body) if op.startswith(".LBB")}
    path, i, seen = [], 0, set()
    while True:
        assert i < len(body) and i not in seen, f"{what}: the walk left the loop or runs in a circle at line {i}"
        seen.add(i)
        op, rest = body[i]
        if op == "s_branch":
            if rest.strip() == top:
                break
            assert rest.strip() in at and at[rest.strip()] > i, f"{what}: a branch out of the loop or backwards: {rest}"
            i = at[rest.strip()]
            continue
        path.append((op, rest))
        i += 1
    n_mfma = sum(op.startswith("v_mfma") for op, _ in path)
    assert n_mfma == 64 + 32, f"{what}: the walked path holds {n_mfma} MFMAs, not a backward (64) and a forward (32)"
    return path


def _lgkm(op, rest):
    if op != "s_waitcnt":
        return None
    m = re.search(r"lgkmcnt\((\d+)\)", rest)
    if m:
        return int(m.group(1))
    assert "vmcnt" in rest or "expcnt" in rest, f"a wait this check cannot read: s_waitcnt {rest}"
    return None


def check_lds_waits(text, declared=None, alter=None):
    """alter = (instantiation or None for all, fn): fn(body) replaces that instantiation's worker loop [(mnemonic, operands)] first."""
    kernels = _kernels(text)
    assert set(kernels) == INSTANCES, f"instantiations found: {sorted(kernels)}"
    for inst, lines in sorted(kernels.items()):
        what = f"{inst} workers"
        R, R_k, counts = (declared or _declared)(inst[2])
        body = _worker_loop(lines, what)
        if alter and alter[0] in (None, inst):
            body = alter[1](list(body))
        for op, rest in body:
            assert not op.startswith("scratch_"), f"{what}: a scratch access in the tile loop: {op} {rest}"
        path = _iteration(body, what)
        dma = [i for i, (op, _) in enumerate(path) if op == "global_load_lds_dwordx4"]
        assert len(dma) == 4, f"{what}: {len(dma)} row DMAs on the path, not 4"
        # ---- what stands between the loop top and D_3
        head = path[:dma[3]]
        for op, rest in head:
            assert not SMEM.match(op), f"{what}: a scalar memory read shares the counter between the loop top and D_3: {op} {rest}"
            assert not (op.startswith("ds_") and not op.startswith("ds_read")), \
                f"{what}: an LDS operation other than a read between the loop top and D_3: {op} {rest}"
        reads = [i for i, (op, _) in enumerate(head) if op.startswith("ds_read")]
        assert len(reads) == R, f"{what}: {len(reads)} LDS reads between the loop top and D_3, the source declares {R}"
        assert reads[-1] < dma[0], f"{what}: an LDS read behind the first row DMA (the R phase is issued up front)"
        kinds = [head[i][0] for i in reads[R - 4 * SLOT_READS:]]
        assert kinds == ["ds_read2st64_b32", "ds_read2st64_b32", "ds_read_b128"] * 4, f"{what}: the slots' reads are {kinds}"
        # ---- the waits on the counter, in order
        waits = [(i, _lgkm(*head[i])) for i in range(len(head)) if _lgkm(*head[i]) is not None]
        # (hipcc rotates some of the loops: tile_barrier then stands at the top, in front of the first read)
        if waits and waits[0][1] == 0 and head[waits[0][0] + 1][0] == "s_barrier" and waits[0][0] < reads[0]:
            waits = waits[1:]
        assert [c for _, c in waits] == counts, \
            f"{what}: waits on lgkmcnt from the loop top to D_3 (tile_barrier's aside) are {[c for _, c in waits]}, declared {counts}"
        for k in range(4):
            lo = dma[k - 1] if k else reads[-1]
            assert lo < waits[k][0] < dma[k], f"{what}: the wait of D_{k} does not stand between D_{k - 1} and D_{k}"
        mfma_before_last = sum(op.startswith("v_mfma") for op, _ in head[:waits[3][0]])
        assert mfma_before_last == 48, f"{what}: {mfma_before_last} MFMAs in front of slot 3's wait, not three groups"
        # ---- replay: LDS operations return in issue order
        returned, outstanding, covered_by = 0, [], {}
        for i, (op, rest) in enumerate(head + [path[dma[3]]]):
            if op.startswith("ds_read"):
                outstanding.append(i)
            c = _lgkm(op, rest)
            if c is not None and len(outstanding) > c:
                for r in outstanding[:len(outstanding) - c]:
                    covered_by[r] = i
                returned += len(outstanding) - c
                outstanding = outstanding[len(outstanding) - c:]
            if op == "global_load_lds_dwordx4":
                k = dma.index(i)
                assert returned >= R_k[k], \
                    f"{what}: at D_{k} only {returned} of the first {R_k[k]} LDS reads have returned " \
                    f"(the wait in front of it is {R_k[k] - returned} too large)"
                assert returned == R_k[k], \
                    f"{what}: at D_{k} {returned} LDS reads have returned, {returned - R_k[k]} more than the derivation says"
        # ---- nothing names a read's destination between the read and the wait that covers it
        for r in reads:
            dst = _regs(head[r][1].split(",")[0])
            assert dst, f"{what}: destination of {head[r]}"
            for op, rest in head[r + 1:covered_by[r]]:
                assert not (dst & _regs(rest)), \
                    f"{what}: `{op} {rest}` names v{min(dst & _regs(rest))} between its LDS read and the wait that covers it"


def test_emitted_worker_loops_hold_the_declared_lds_reads_and_waits(step_asm):  # noqa: F811
    check_lds_waits(step_asm)


def _at(body, op, rest=None, last=False):
    hits = [i for i, (o, r) in enumerate(body) if o == op and (rest is None or r.strip() == rest)]
    assert hits, f"no `{op} {rest or ''}` in the worker loop"
    return hits[-1 if last else 0]


def _wait(old, new):
    """The loop's wait lgkmcnt(old) with another count (None: removed)."""
    def fn(body):
        i = _at(body, "s_waitcnt", f"lgkmcnt({old})")
        body[i:i + 1] = [("s_waitcnt", f"lgkmcnt({new})")] if new is not None else []
        return body
    return fn


def _insert_before_first_wait(op, rest):
    def fn(body):
        i = _at(body, "s_waitcnt", "lgkmcnt(9)")
        return body[:i] + [(op, rest)] + body[i:]
    return fn


def _last_slot_read(body):
    return max(i for i in range(_at(body, "global_load_lds_dwordx4")) if body[i][0] == "ds_read_b128")


def _read_moved_behind_first_dma(body):
    d = _at(body, "global_load_lds_dwordx4")
    body.insert(d, body.pop(_last_slot_read(body)))
    return body


def _named_early(body):
    r = _last_slot_read(body)                      # slot 3's e4: a copy right behind its read
    reg = min(_regs(body[r][1].split(",")[0]))
    return body[:r + 1] + [("v_mov_b32_e32", f"v{reg}, v{reg}")] + body[r + 1:]


ALTERED = [
    ("the first count one too large", _wait(9, 10), "declared"),
    ("the second count one too large", _wait(6, 7), "declared"),
    ("the third count one too small", _wait(3, 2), "declared"),
    ("a drain in front of the first DMA", _wait(9, 0), "declared"),
    ("a wait removed", _wait(6, None), "declared"),
    ("a read moved behind the first DMA", _read_moved_behind_first_dma, "behind the first row DMA"),
    ("a destination register named early", _named_early, "between its LDS read and the wait that covers it"),
    ("a scratch reload", _insert_before_first_wait("scratch_load_dword", "v1, off, s0"), "scratch access"),
    ("a scalar memory read", _insert_before_first_wait("s_load_dword", "s0, s[4:5], 0x0"), "scalar memory read"),
    ("an LDS write", _insert_before_first_wait("ds_write_b32", "v1, v2"), "other than a read"),
]


@pytest.mark.parametrize("inst", [(0, 0, 0), (1, 0, 1)], ids=["plain", "packed"])
@pytest.mark.parametrize("what,fn,message", ALTERED, ids=[a[0] for a in ALTERED])
def test_the_checker_fails_an_altered_copy_of_the_emitted_code(step_asm, inst, what, fn, message):  # noqa: F811
    with pytest.raises(AssertionError, match=re.escape(message)):
        check_lds_waits(step_asm, alter=(inst, fn))


def test_the_replay_refuses_counts_that_code_and_declaration_agree_on_but_are_off(step_asm):  # noqa: F811
    """A count raised by one everywhere - in the code AND in what the check takes for declared: only the replay of the
    in-order counter can tell that slot j's last read may still be in flight at D_j; lowered by one, that the wait
    retires a read of the next slot."""
    for delta, message in ((1, "(the wait in front of it is 1 too large)"), (-1, "1 more than the derivation says")):
        def shifted(body, delta=delta):
            return [(op, re.sub(r"lgkmcnt\((9|6|3)\)", lambda m: f"lgkmcnt({int(m.group(1)) + delta})", rest))
                    if op == "s_waitcnt" else (op, rest) for op, rest in body]

        def declared(packed, delta=delta):
            R, R_k, counts = _declared(packed)
            return R, R_k, [c + delta if c else 0 for c in counts]
        with pytest.raises(AssertionError, match=re.escape(message)):
            check_lds_waits(step_asm, declared, alter=(None, shifted))
