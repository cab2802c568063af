"""Test aids for the state a kernel FINDS, as opposed to the state it is given (a plain module, not a conftest: test
modules import what they need).

LDS.  What a kernel reads from LDS before it has written it is whatever the last workgroup on that CU left there:
mostly zeros in a fresh test process, another layer's tile in production.  The `lds_pattern` fixture makes it ONE known
bit pattern: while it is active, every entry point that goes through recman_amd._lib.call (ops, engine, optim, metrics
and dist all do) gets ops.debug_lds_fill(pattern) enqueued on the current stream directly in front of it; the
rm_debug_* aids themselves are left alone.  An entry point that launches several kernels is poisoned in front of the
first one only - the later kernels see what the earlier ones left, as they do in production.

`run_patterns` runs one case under four patterns, in this order:
  ZERO 0x00000000 and ONE 0x00000001 first - a stale word that is used as an integer (a count, an offset, a row
       number: optim, route, metrics, gauc and the step keep such words in LDS) differs between the two while both
       are still in range, so the case fails on a bit comparison and no wild address reaches the card;
  QNAN 0x7fc00000 - 0 x stale is NaN, not 0;
  HUGE 0x7e967699 (about 1e38) - what max(x, 0) and comparisons launder out of a NaN still overflows or dominates.
QNAN and HUGE run only if ZERO and ONE agreed bit for bit; then all four must pass the family's own float64 check and
be bit-identical.

HBM.  `poisoned` is a NaN-filled output, `guarded(n)` an n-float NaN-filled workspace between two bands of a sentinel
bit pattern (`assert_guards_intact` checks the bands: a kernel that writes past the size its *_workspace() function
reports changes them).
"""
import pytest
import torch

ZERO, ONE, QNAN, HUGE = 0x00000000, 0x00000001, 0x7FC00000, 0x7E967699
PATTERNS = (ZERO, ONE, QNAN, HUGE)
NAMES = {ZERO: "ZERO", ONE: "ONE", QNAN: "QNAN", HUGE: "HUGE"}

GUARD = 64                 # floats in each band
GUARD_BITS = 0x7FA5C3E1    # a signalling-NaN payload nothing computes
_ACTIVE = []               # the state of the lds_pattern fixture of the running test


@pytest.fixture
def lds_pattern(monkeypatch, hip_lib):
    """-> state: state["pattern"] (None = no fill) is written into all of every CU's LDS in front of every entry
    point called through _lib.call; state["seen"] collects the entry points' names, state["fills"] counts."""
    from recman_amd import _lib, ops

    state = {"pattern": None, "seen": set(), "fills": 0}
    call = _lib.call

    def filled(name, *args):
        if not name.startswith("rm_debug_"):
            state["seen"].add(name)
            if state["pattern"] is not None:
                call("rm_debug_lds_fill", int(state["pattern"]) & 0xFFFFFFFF, ops._stream())
                state["fills"] += 1
        return call(name, *args)

    monkeypatch.setattr(_lib, "call", filled)
    _ACTIVE.append(state)
    yield state
    _ACTIVE.remove(state)


def _leaves(x, path="out"):
    """The tensors (and plain numbers) of a nested result, with a name each."""
    if x is None:
        return
    if torch.is_tensor(x):
        yield path, x
    elif isinstance(x, dict):
        for k in x:
            yield from _leaves(x[k], f"{path}[{k!r}]")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _leaves(v, f"{path}[{i}]")
    elif isinstance(x, (bool, int, float)):
        yield path, torch.tensor(float(x), dtype=torch.float64)
    else:
        raise TypeError(f"{path}: {type(x).__name__} is neither a tensor, a number nor a container of them")


def snapshot(x):
    """{name: a CPU copy of each tensor of a nested result}: later runs may reuse the buffers."""
    return {n: t.detach().clone().cpu().contiguous() for n, t in _leaves(x)}


def same_bits(a, b, what):
    """Two snapshots hold the same tensors with the same bits (NaNs compared by payload, -0.0 differs from +0.0)."""
    assert list(a) == list(b), f"{what}: the runs returned different results: {sorted(set(a) ^ set(b))}"
    for n in a:
        x, y = a[n], b[n]
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {n} changed its shape or type"
        if x.numel() == 0:
            continue
        bx, by = x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)
        if not torch.equal(bx, by):
            size = x.element_size()
            bad = (bx != by).reshape(-1, size).any(1).nonzero().reshape(-1)
            i = int(bad[0])
            raise AssertionError(f"{what}: {n} differs in {bad.numel()} of {x.numel()} elements, first at flat index "
                                 f"{i}: {x.reshape(-1)[i].item()!r} against {y.reshape(-1)[i].item()!r}")


def run_patterns(run, check=None, what=""):
    """run() under each LDS pattern (the test uses the lds_pattern fixture): ZERO and ONE first, which must agree bit
    for bit before QNAN and HUGE run; then every run passes check(result) and all four are bit-identical.
    -> {pattern: snapshot}."""
    assert len(_ACTIVE) == 1, "run_patterns needs the lds_pattern fixture"
    state, patterns = _ACTIVE[0], PATTERNS
    snaps, results = {}, {}
    try:
        for p in patterns:
            state["pattern"] = p
            results[p] = run()
            torch.cuda.synchronize()
            snaps[p] = snapshot(results[p])
            if check is not None and p in (QNAN, HUGE):
                check(results[p])
            if p == ONE:
                same_bits(snaps[ZERO], snaps[ONE], f"{what}LDS filled with ZERO against LDS filled with ONE")
                if check is not None:
                    check(results[ZERO])
                    check(results[ONE])
            torch.cuda.synchronize()
    finally:
        state["pattern"] = None
    first = patterns[0]
    for p in patterns[1:]:
        same_bits(snaps[first], snaps[p], f"{what}LDS filled with {NAMES[first]} against LDS filled with {NAMES[p]}")
    return snaps


def poisoned(*shape, dtype=torch.float32):
    """A NaN-filled device tensor: an output the call has to overwrite fully."""
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def guarded(n, fill=float("nan")):
    """-> (view, buffer): an n-float, 16-byte-aligned, `fill`-filled view between two GUARD-float bands of
    GUARD_BITS.  n is what the kernel's *_workspace() function reports, exactly."""
    n = int(n)
    buf = torch.full((GUARD + n + GUARD,), GUARD_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    view = buf[GUARD:GUARD + n]
    view.fill_(fill)
    assert view.data_ptr() % 16 == 0
    return view, buf


def assert_guards_intact(buf, what=""):
    bits = buf.view(torch.int32)
    n = bits.numel() - 2 * GUARD
    assert bool((bits[:GUARD] == GUARD_BITS).all()), f"{what}: the floats in front of the workspace were written"
    assert bool((bits[GUARD + n:] == GUARD_BITS).all()), \
        f"{what}: floats past the size the workspace function reports were written"


def padded(t, pad, fill=float("nan")):
    """-> (view, buffer): a device copy of the 2-D float32 `t` as the leading columns of rows `pad` floats longer,
    the pad columns holding `fill` (NaN: a kernel that reads them poisons its output, `assert_pads_nan` shows one
    that wrote them)."""
    M, N = t.shape
    buf = torch.full((M, N + pad), fill, dtype=torch.float32, device="cuda")
    buf[:, :N] = t.to(device="cuda", dtype=torch.float32)
    return buf[:, :N], buf


def assert_pads_nan(buf, N, what=""):
    assert bool(torch.isnan(buf[:, N:]).all()), f"{what}: pad columns past {N} were written"
