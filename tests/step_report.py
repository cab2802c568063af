"""Where a bad element of rm_deepfm_step's outputs (csrc/step.hip) came from: test infrastructure, CPU only.

A failure of tests/test_gpu_step_waits.py may not be rerun to learn more, so ONE failure has to say everything: which
outputs were hit, and for every bad element which block computed it, as which of the block's tiles (a block's first
three tiles read ring buffers that nothing has written yet - the fill), in which lane, and - for row gradients -
which worker wave and slot owns the field.  `Findings` collects boolean masks over ALL outputs of a run and raises
once; tests/test_step_waits_host.py pins the arithmetic below with synthetic masks.

The kernel's arithmetic, restated (each piece cited against the source by `_cite`):
 * launch: ntiles = ceil(B / 16) tiles of 16 examples on nblk = min(ntiles, 256) blocks; block k runs tiles
   k, k + nblk, ...: example b is lane n = b % 16 of tile b // 16 = block (b // 16) % nblk, its tile (b // 16) // nblk;
 * slot map: field f < 21 is slot f // 7 of worker f % 7; the last round skips worker 3; the dense inputs are the
   pseudo-field F (rows 16 F .. 16 F + Dn - 1 of dW0).
"""
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKERS, SLOTS, RING, TILE, MAX_BLOCKS, D = 7, 4, 3, 16, 256, 16
CAP = 32  # bad elements listed per output (the count is always given)
PER_EXAMPLE = ("logit", "pred", "dlogit")


def _cite(snippet):
    with open(os.path.join(ROOT, "recman_amd", "csrc", "step.hip")) as f:
        src = " ".join(f.read().split())
    assert " ".join(snippet.split()) in src, f"csrc/step.hip no longer contains `{snippet}`: re-derive tests/step_report.py"


def cite_all():
    _cite("return j < 3 ? 7 * j + w : (w < 3 ? 21 + w : (w > 3 ? 20 + w : -1));")
    _cite("const int64_t ntiles = (B + 15) / 16;")
    _cite("const int nblk = rm_grid_cap(ntiles, 256);")
    _cite("const int T = (int)((ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x);")
    _cite("constexpr int kRing = 3;")


def slot_field(w, j):
    return 7 * j + w if j < 3 else (21 + w if w < 3 else (20 + w if w > 3 else -1))


def slot_map(F, Dn):
    """field -> (worker, slot) for the fields 0..F-1 and, with dense inputs, the pseudo-field F."""
    at = {}
    for w in range(WORKERS):
        for j in range(SLOTS):
            f = slot_field(w, j)
            if 0 <= f < F or (f == F and Dn > 0):
                assert f not in at
                at[f] = (w, j)
    return at


def launch(B):
    ntiles = -(-B // TILE)
    return ntiles, min(ntiles, MAX_BLOCKS)


def locate(b, B):
    """(block, tile within the block, lane n, tile is one of the block's first three) of example b."""
    _, nblk = launch(B)
    t = b // TILE
    return t % nblk, t // nblk, b % TILE, t // nblk < RING


def _where(b, B):
    blk, tile, n, fill = locate(b, B)
    return f"b {b} = block {blk} tile {tile} ({'fill: first three' if fill else 'steady'}) lane n {n}"


def _first(idx):
    idx = [int(i) for i in idx]
    return idx[:CAP], len(idx)


def _vals(values, index):
    """' got x / y' for the element `index` of every tensor in `values` (one run, or two runs side by side)."""
    if not values:
        return ""
    return " [" + " / ".join(f"{float(v[index]):.9g}" for v in values) + "]"


def describe(key, mask, B, F, Dn, pos=None, values=()):
    """Lines that place the True elements of `mask` (the shape of output `key`) in the kernel.  values: tensors of the
    output's shape whose elements are quoted beside each place.  pos [B, F]: the packed form's positions (d_rows is
    then the send buffer [rows, 20], a row's place is the occurrence that addresses it)."""
    mask = mask.detach().cpu()
    values = [v.detach().cpu() for v in values]
    n_bad = int(mask.sum())
    if n_bad == 0:
        return []
    at = slot_map(F, Dn)
    out = [f"{key}: {n_bad} of {mask.numel()} elements"]
    if key in PER_EXAMPLE:
        idx, n = _first(mask.reshape(B).nonzero().reshape(-1))
        out += [f"  {_where(b, B)}{_vals(values, b)}" for b in idx]
        out += [f"  ... and {n - len(idx)} more examples"] if n > len(idx) else []
    elif key == "d_rows":
        if pos is None:
            occ = mask.reshape(B, F, -1).any(2)
            elem = lambda b, f: (b, f, int(mask.reshape(B, F, -1)[b, f].nonzero()[0]))
        else:
            rows = mask.reshape(mask.shape[0], -1).any(1)
            occ = rows[pos.reshape(-1)].reshape(B, F)
            stray = rows.clone()
            stray[pos.reshape(-1)] = False
            if bool(stray.any()):
                idx, n = _first(stray.nonzero().reshape(-1))
                out.append(f"  {n} rows of the send buffer that no occurrence addresses, first {idx}")
            elem = lambda b, f: (int(pos[b, f]), int(mask[int(pos[b, f])].nonzero()[0]))
        fields = occ.any(0).nonzero().reshape(-1).tolist()
        out.append("  fields " + ", ".join(f"{f} (worker {at[f][0]} slot {at[f][1]})" for f in fields))
        idx, n = _first(occ.any(1).nonzero().reshape(-1))
        for b in idx:
            fs = occ[b].nonzero().reshape(-1).tolist()
            out.append(f"  {_where(b, B)} fields {fs}{_vals(values, elem(b, fs[0]))}")
        out += [f"  ... and {n - len(idx)} more examples"] if n > len(idx) else []
    elif key == "dW0":
        rows = mask.reshape(mask.shape[0], -1).any(1).nonzero().reshape(-1)
        fields = sorted({int(k) // D for k in rows})
        for f in fields:
            ks = [int(k) for k in rows if int(k) // D == f]
            name = f"field {f}" if f < F else "the dense pseudo-field"
            out.append(f"  rows {ks[0]}..{ks[-1]} ({len(ks)} of them): {name} (worker {at[f][0]} slot {at[f][1]})")
        i = tuple(int(x) for x in mask.nonzero()[0])
        out.append(f"  first bad element {i}{_vals(values, i)}")
    else:  # the head's block-reduced outputs
        idx, n = _first(mask.reshape(-1).nonzero().reshape(-1))
        out.append(f"  (summed over every block by the head wave) elements {idx}"
                   + "".join(_vals([v.reshape(-1) for v in values], i) for i in idx[:4]))
    return out


class Findings:
    """Everything that is wrong with one run (or between two), collected over all outputs before anything raises."""

    def __init__(self, what, B, F, Dn, pos=None):
        self.what, self.B, self.F, self.Dn, self.pos = what, B, F, Dn, pos
        self.lines = []

    def add(self, reason, key, mask, values=()):
        if not bool(mask.any()):  # (on the mask's device: nothing is copied for an output that is good)
            return
        lines = describe(key, mask, self.B, self.F, self.Dn, self.pos if key == "d_rows" else None, values)
        if lines:
            self.lines += [f"[{reason}] {lines[0]}"] + lines[1:]

    def note(self, text):
        self.lines.append(text)

    def text(self):
        ntiles, nblk = launch(self.B)
        head = (f"{self.what}: B {self.B} F {self.F} Dn {self.Dn}: {ntiles} tiles on {nblk} blocks, "
                f"{-(-ntiles // nblk)} or fewer tiles per block")
        return "\n".join([head] + self.lines)

    def raise_if_any(self):
        if self.lines:
            raise AssertionError(self.text())


def tolerance_masks(o, ref, pos=None):
    """name -> mask of the elements outside the tolerances tests/test_gpu_step_kernel.py holds the kernel to (logit /
    pred 1e-5 absolute, loss _close's defaults, the gradients _close_grad's 2e-5 of max(|want|, 0.1 max|want|));
    o: name -> float32 CPU tensor, ref: the float64 reference.  A NaN is outside every tolerance.  The packed form's
    send buffer (pos given) is compared in its addressed rows' first 16 columns."""
    masks = {}
    for k, got in o.items():
        want = ref.get(k)
        if want is None:
            continue
        got, want = got.double(), want.double()
        if k == "d_rows" and pos is not None:
            m = torch.zeros(got.shape, dtype=torch.bool)
            p = pos.reshape(-1)
            g, w = got[p][:, :D], want.reshape(-1, D)
            tol = 2e-5 * torch.clamp(w.abs(), min=0.1 * float(w.abs().max()))
            sub = torch.zeros(p.numel(), got.shape[1], dtype=torch.bool)
            sub[:, :D] = ~((g - w).abs() <= tol)
            m[p] = sub
            masks[k] = m
            continue
        got = got.reshape(want.shape)
        if k in ("logit", "pred"):
            tol = torch.full_like(want, 1e-5)
        elif k == "loss":
            tol = torch.full_like(want, 1e-6 + 1e-5 * max(1.0, float(want.abs().max())))
        else:
            tol = 2e-5 * torch.clamp(want.abs(), min=0.1 * float(want.abs().max()))
        masks[k] = ~((got - want).abs() <= tol)
    return masks
