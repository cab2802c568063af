"""GPU: the skinny-MLP kernels of csrc/mlp.hip - rm_mlp_fwd, rm_embed_mlp_fwd, rm_mlp_bwd (dh chain, dX / dW0 kernel,
small gradients, finishing kernel) and the fused training head rm_mlp_tail - called through recman_amd/ops.py and held,
stage by stage, to the float64 references of tests/mlp_ref.py.

Method.  Every output is compared with the float64 function of the inputs that PRODUCED it, intermediates taken from
the kernel itself: h_l from the kernel's h_{l-1}, dh_{l-1} from the kernel's dh_l and h_{l-1}, the gradients from the
kernel's h / dh / g.  Each link is held to front_refs.sum_bound(n, sum|terms|) with the n its reference states; the
chain is verified by induction, and no example or element is left out of any comparison.  Outputs that pass through
expf / logf (pred, dlogit, loss) use front_refs.close (rtol 1e-5, atol 1e-6).

Guard bands.  Every per-example input is a contiguous slice arena[G : G + B] of a larger tensor whose other rows are
NaN (ids and integer labels: a value no table or loss has); every output is such a slice of a sentinel-filled arena,
and an output that a later kernel READS (h, dh, dlogit, E, fm_sum, the branch logits) has NaN for its sentinel, so
that it is NaN-guarded as an input too; the workspace is NaN before each call.  Afterwards the guard rows of every output hold the sentinel bit for bit, the
padded columns >= H_l of h_out[l] / dh[l] are exactly 0 and every result is finite - a read past row B that reaches
an MFMA shows up as NaN instead of vanishing against a zero factor.  Everything stays inside allocated memory.

Paths.  Each case restates the launch arithmetic of the C++ it cites and asserts the path its shape reaches (`_cite`
fails when the source text changes, the asserts when the numbers do).

The largest error / bound ratio seen per kernel is collected in front_refs.RATIOS and printed by the last test."""
import os

import pytest
import torch

from recman_amd import _lib, ops
from tests import front_refs as R
from tests import mlp_cases as MC
from tests import mlp_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, I64 = torch.float32, torch.float64, torch.int64
NAN = float("nan")
SENT = -777.25
G = 40            # guard rows on either side: more than the 31 rows a 32-example tile can reach past B
BAD_ID = 1 << 40  # guard value of id arenas: no table has such a row
BAD_LABEL = 7777  # guard value of integer-label arenas


def cdiv(a, b):
    return -(-a // b)


_SRC = {}


def _cite(name, snippet):
    """The launch code a case relies on, as it stands in recman_amd/csrc/<name> (whitespace-insensitive)."""
    if name not in _SRC:
        with open(os.path.join(ROOT, "recman_amd", "csrc", name)) as f:
            _SRC[name] = " ".join(f.read().split())
    assert " ".join(snippet.split()) in _SRC[name], f"csrc/{name} no longer contains `{snippet}`: re-derive this case"


# ================================================================================================ launch arithmetic
LDS_CAP = 160 * 1024


def _kp(K):
    _cite("mlp.hip", "const int Kp = ((K + 63) / 64) * 64;")
    return (K + 63) // 64 * 64


def _bwd_smem(K, Ds):
    _cite("mlp.hip", "constexpr int kLDT = 36;")
    _cite("mlp.hip", "return (size_t)(Kp * 36 + 8 * 32 * kLDT + 8 * 32 * 33 + 8 * 32 * Ds) * sizeof(float);")
    return (_kp(K) * 36 + 8 * 32 * 36 + 8 * 32 * 33 + 8 * 32 * Ds) * 4


def _tile_kinds(FD, Dn):
    """One letter per 32-column k-tile of mlp_bwd_kernel, by the three wave-uniform tests of load_ktile:
    E all-in-xe loader; S the straddling (per-lane-branch) loader; behind xe, raw buffer loads: D a tile with dense
    columns, P pure padding behind them, Z padding with Dn == 0 - a descriptor of zero records on xe."""
    _cite("mlp.hip", "const int nkt = Kp / 32;")
    _cite("mlp.hip", "if (kb + 32 <= FD) {")
    _cite("mlp.hip", "if (kb >= FD) {")
    _cite("mlp.hip", "Dn > 0 ? (int)(rows_t * Dn * 4) : 0, 0x00020000);")
    _cite("mlp.hip", "vo[e] = kk < Dn ? ((lane >> 3) * Dn + kk) * 4 : 0x7ffffff0;")
    _cite("mlp.hip", "if (k + 3 < FD) {")
    out = ""
    for kb in range(0, _kp(FD + Dn), 32):
        if kb + 32 <= FD:
            out += "E"
        elif kb >= FD:
            out += "Z" if Dn == 0 else ("D" if kb < FD + Dn else "P")
        else:
            out += "S"
    return out


def _paths(FD, Dn, B, D=0):
    """What a call of rm_mlp_fwd / rm_mlp_bwd with these sizes launches."""
    K = FD + Dn
    Kp = _kp(K)
    _cite("mlp.hip", "const int nch = Kp / 64;")
    _cite("mlp.hip", "for (int ch = 0; ch < nch; ch += 2) {")   # two chunks per trip: odd and even nch end differently
    _cite("mlp.hip", "const bool split14 = nkt == 14;")
    _cite("mlp.hip", "#define RM_MLP_FWD_WAVES 8")
    _cite("mlp.hip", "dim3 grid((unsigned)rm_grid_cap((ntiles + RM_MLP_FWD_WAVES - 1) / RM_MLP_FWD_WAVES, 256));")
    _cite("mlp.hip", "for (int64_t tile = tile0; tile < ntiles; tile += (int64_t)gridDim.x * NW) {")
    _cite("mlp.hip", "const int nblk = rm_grid_cap(ntiles, 256);")
    _cite("mlp.hip", "for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {")
    _cite("mlp.hip", "const int64_t ex_next = (tile + gridDim.x < ntiles ? tile + gridDim.x : tile) * 32;")
    _cite("mlp.hip", "const int s_lds = (fm_sum != nullptr && mlp_bwd_smem(K, D) <= 160 * 1024) ? 1 : 0;")
    _cite("mlp.hip", "const size_t smem = mlp_bwd_smem(K, s_lds ? D : 0);")
    _cite("mlp.hip", "const bool s_pf = s_lds && D == 16;")
    ntiles = cdiv(B, 32)
    s_lds = bool(D) and _bwd_smem(K, D) <= LDS_CAP
    fm = "none" if not D else ("s_pf" if s_lds and D == 16 else ("lds" if s_lds else "global"))
    fwd_blocks, bwd_blocks = min(cdiv(ntiles, 8), 256), min(ntiles, 256)
    return dict(Kp=Kp, nkt=Kp // 32, nch=Kp // 64, split14=Kp // 32 == 14, tiles=_tile_kinds(FD, Dn), fm=fm,
                smem=_bwd_smem(K, D if s_lds else 0), ntiles=ntiles, fwd_blocks=fwd_blocks, bwd_blocks=bwd_blocks,
                fwd_sweeps=cdiv(ntiles, 8 * fwd_blocks), bwd_sweeps=cdiv(ntiles, bwd_blocks))


# ====================================================================================================== guard bands
class Arena:
    """A tensor [n + 2 G, ...] filled with `fill`; .v is its contiguous slice [G : G + n]."""

    def __init__(self, shape, fill=SENT, dtype=F32, data=None):
        n = shape[0]
        self.n, self.fill = n, fill
        self.full = torch.full((n + 2 * G, *shape[1:]), fill, device="cuda", dtype=dtype)
        self.v = self.full[G:G + n]
        if data is not None:
            self.v.copy_(data)

    def check(self, what):
        want = torch.full_like(self.full[:G], self.fill)
        R.assert_bits(self.full[:G], want, f"{what}: guard rows before the output")
        R.assert_bits(self.full[G + self.n:], want, f"{what}: guard rows behind the output")


def _in(t, fill=NAN):
    """An input tensor as the slice of a guarded arena (None stays None)."""
    return None if t is None else Arena(tuple(t.shape), fill, t.dtype, t).v


def _outs(*shapes, fill=SENT):
    return [Arena(s, fill) for s in shapes]


def _zero_pad(a, H, what):
    assert not bool(a[:, H:].any()), f"{what}: columns >= {H} are not exactly 0"


class Case:
    """The device tensors of one case: guarded inputs, plain parameters."""

    def __init__(self, FD, Dn, B, hidden, act, D=0, seed=0):
        p = MC.make_mlp_inputs(FD, Dn, B, hidden, seed)
        self.FD, self.Dn, self.B, self.hidden, self.act, self.D, self.NL = FD, Dn, B, tuple(hidden), act, D, len(hidden)
        self.xe, self.xd, self.g = _in(p["xe"]), _in(p["xd"]), _in(p["g"])
        self.Ws, self.bs = [W.cuda() for W in p["Ws"]], [b.cuda() for b in p["bs"]]
        self.w_out, self.w0 = p["w_out"].cuda(), p["w0"].cuda()
        self.S = _in(MC.fm_sum32(p["xe"], D)) if D else None
        self.x = self.xe if self.xd is None else torch.cat([self.xe, self.xd], 1)
        self.what = f"FD={FD} Dn={Dn} B={B} hidden={self.hidden} {act} D={D}"


class Fwd:
    """rm_mlp_fwd into guarded outputs."""

    def __init__(self, c, tail=None, run=True):
        # (NaN sentinels: rm_mlp_bwd reads h, rm_logit_loss the logit)
        self.h, (self.logit,) = _outs(*[(c.B, 32)] * c.NL, fill=NAN), _outs((c.B,), fill=NAN)
        if run:
            ops.mlp_fwd(c.xe, c.xd, c.Ws, c.bs, c.w_out, c.w0, c.act, [a.v for a in self.h], self.logit.v, tail=tail)

    def hv(self):
        return [a.v for a in self.h]


def check_fwd(c, f, key="mlp_fwd"):
    """h_l from the kernel's h_{l-1} (n = K_l + 1), the logit from its h_last (n = H + 1), padding, guards."""
    for l, H in enumerate(c.hidden):
        ref, ab = M.layer_ref(c.x if l == 0 else f.h[l - 1].v, c.Ws[l], c.bs[l], c.act)
        R.assert_within(f.h[l].v[:, :H], ref, R.sum_bound(c.Ws[l].shape[0] + 1, ab), f"{c.what}: h{l}", key=f"{key}: h")
        _zero_pad(f.h[l].v, H, f"{c.what}: h{l}")
        f.h[l].check(f"{c.what}: h{l}")
    ref, ab = M.logit_ref(f.h[-1].v, c.w_out, c.w0)
    R.assert_within(f.logit.v, ref, R.sum_bound(c.hidden[-1] + 1, ab), f"{c.what}: logit", key=f"{key}: logit")
    f.logit.check(f"{c.what}: logit")


class Bwd:
    """rm_mlp_bwd into guarded outputs on a NaN-filled workspace."""

    def __init__(self, c, h, g=None, tail=None, dh=None, ws=None, skip=(), xd_wsum=False, g_sum=False, stream=False,
                 fm=True):
        self.g = c.g if g is None else g
        self.d_rows, self.dwo, self.dw0 = _outs((c.B, c.FD), (c.hidden[-1],), (1,))
        self.dh = _outs(*[(c.B, 32)] * c.NL, fill=NAN) if dh is None else dh   # (read again by the same call)
        self.dW, self.db = _outs(*[tuple(W.shape) for W in c.Ws]), _outs(*[(H,) for H in c.hidden])
        self.dxd = Arena((c.Dn,)) if xd_wsum else None
        self.dgs = Arena((1,)) if g_sum else None
        self.ws = torch.empty(ops.mlp_bwd_workspace(c.FD, c.Dn), device="cuda") if ws is None else ws
        self.ws.fill_(NAN)
        self.skip = skip
        opt = lambda name, a: None if name in skip else a
        ops.mlp_bwd(c.xe, c.xd, c.Ws, c.w_out, c.act, self.g, h, self.d_rows.v, [a.v for a in self.dh],
                    [a.v for a in self.dW], self.ws, fm_sum=c.S if fm else None,
                    db=opt("db", [a.v for a in self.db]), d_w_out=opt("d_w_out", self.dwo.v),
                    d_w0_out=opt("d_w0_out", self.dw0.v), d_xd_wsum=None if self.dxd is None else self.dxd.v,
                    d_g_sum=None if self.dgs is None else self.dgs.v, tail=tail, stream_d_rows=stream)

    def outputs(self):
        o = dict(d_rows=self.d_rows, d_w_out=self.dwo, d_w0_out=self.dw0)
        for l in range(len(self.dh)):
            o.update({f"dh{l}": self.dh[l], f"dW{l}": self.dW[l], f"db{l}": self.db[l]})
        if self.dxd is not None:
            o["d_xd_wsum"] = self.dxd
        if self.dgs is not None:
            o["d_g_sum"] = self.dgs
        return {k: v for k, v in o.items() if not any(k.startswith(s) for s in self.skip)}


def check_bwd(c, h, b, fm=True, key="mlp_bwd"):
    """The chain link by link from the kernel's own dh_l and h_{l-1}; d_rows, dW, db, d_w_out, the g sums from the
    kernel's h / dh / g.  The n of every bound is the one the reference states."""
    B, NL, w = c.B, c.NL, c.what
    ref, ab = M.dh_last_ref(b.g, c.w_out, h[-1], c.act)
    R.assert_within(b.dh[-1].v[:, :c.hidden[-1]], ref, R.sum_bound(c.hidden[-1] + 1, ab), f"{w}: dh{NL - 1}",
                    key=f"{key}: dh")                                                          # n = H + 1
    for l in range(NL - 1, 0, -1):
        ref, ab = M.dh_prev_ref(b.dh[l].v, c.Ws[l], h[l - 1], c.act)
        R.assert_within(b.dh[l - 1].v[:, :c.hidden[l - 1]], ref, R.sum_bound(c.hidden[l] + 1, ab), f"{w}: dh{l - 1}",
                        key=f"{key}: dh")                                                      # n = H_l + 1
    for l, H in enumerate(c.hidden):
        _zero_pad(b.dh[l].v, H, f"{w}: dh{l}")
    S = c.S if fm else None
    ref, ab = M.d_rows_ref(b.dh[0].v, c.Ws[0], c.FD, b.g, S, c.xe if S is not None else None)
    R.assert_within(b.d_rows.v, ref, R.sum_bound(c.hidden[0] + 2, ab), f"{w}: d_rows", key=f"{key}: d_rows")  # n = H0 + 2
    ref, ab = M.dW0_ref(c.x, b.dh[0].v)
    H0 = c.hidden[0]
    R.assert_within(b.dW[0].v, ref[:, :H0], R.sum_bound(B, ab[:, :H0]), f"{w}: dW0", key=f"{key}: dW0")      # n = B
    for l in range(1, NL):
        ref, ab = M.dW_ref(h[l - 1], b.dh[l].v)
        Hp, Hl = c.hidden[l - 1], c.hidden[l]
        R.assert_within(b.dW[l].v, ref[:Hp, :Hl], R.sum_bound(B, ab[:Hp, :Hl]), f"{w}: dW{l}", key=f"{key}: dW_l")
    if "db" not in b.skip:
        for l, H in enumerate(c.hidden):
            ref, ab = M.db_ref(b.dh[l].v)
            R.assert_within(b.db[l].v, ref[:H], R.sum_bound(B, ab[:H]), f"{w}: db{l}", key=f"{key}: db")
    if "d_w_out" not in b.skip:
        ref, ab = M.d_w_out_ref(h[-1], b.g)
        H = c.hidden[-1]
        R.assert_within(b.dwo.v, ref[:H], R.sum_bound(B, ab[:H]), f"{w}: d_w_out", key=f"{key}: d_w_out")
    ref, ab = M.sum_g_ref(b.g)
    if "d_w0_out" not in b.skip:
        R.assert_within(b.dw0.v, ref, R.sum_bound(B, ab), f"{w}: d_w0_out", key=f"{key}: sum g")
    if b.dgs is not None:
        R.assert_within(b.dgs.v, ref, R.sum_bound(B, ab), f"{w}: d_g_sum", key=f"{key}: sum g")
    if b.dxd is not None:
        ref, ab = M.d_xd_wsum_ref(c.xd, b.g)
        R.assert_within(b.dxd.v, ref, R.sum_bound(B, ab), f"{w}: d_xd_wsum", key=f"{key}: d_xd_wsum")
    for name, a in b.outputs().items():
        a.check(f"{w}: {name}")


def fwd_bwd(c, **kw):
    f = Fwd(c)
    check_fwd(c, f)
    b = Bwd(c, f.hv(), **kw)
    check_bwd(c, f.hv(), b)
    return f, b


def _same(b1, b2, what):
    o1, o2 = b1.outputs(), b2.outputs()
    for k in o1:
        if k in o2:
            R.assert_bits(o2[k].v, o1[k].v, f"{what}: {k}")


# ====================================================================================== 1. loaders, chunk counts, grids
#                   k-tiles of the backward       nch
LOADER_PATHS = {
    (0, 1): ("DP", 1),                       # no embedding part: one dense-only buffer tile and a padding tile
    (0, 37): ("DD", 1),                      # two dense-only tiles (Dn > 32)
    (0, 448): ("D" * 14, 7),                 # fourteen of them, under split14
    (4, 0): ("SZ", 1),                       # one partial chunk: xe ends inside a float4 column group of tile 0
    (64, 0): ("EE", 1),                      # exactly one chunk
    (128, 0): ("EEEE", 2),                   # two whole chunks
    (60, 4): ("ES", 1),                      # the xe / xd boundary on a float4 inside a chunk
    (64, 1): ("EEDP", 2),                    # second chunk dense-only
    (96, 0): ("EEEZ", 2),                    # padding tile behind xe with Dn == 0: the zero-record descriptor
    (112, 3): ("EEES", 2),                   # FD % 32 == 16: the straddling loader
    (432, 16): ("E" * 13 + "S", 7),          # ... under split14
    (192, 40): ("E" * 6 + "DD", 4),          # Dn > 32: two dense tiles behind xe
    (256, 33): ("E" * 8 + "DD", 5),
    (320, 64): ("E" * 10 + "DD", 6),
    (416, 13): ("E" * 13 + "D", 7),          # split14, tile 13 dense-only and ragged
    (416, 32): ("E" * 13 + "D", 7),          # split14, tile 13 dense-only and full
    (448, 0): ("E" * 14, 7),                 # split14, tile 13 carries dX too
    (128, 5): ("EEEEDP", 3),
}


def test_the_loader_shapes_reach_what_they_claim():
    assert set(LOADER_PATHS) == set(MC.LOADER_SHAPES)
    seen_nch, seen_tiles = set(), ""
    for (FD, Dn), (tiles, nch) in LOADER_PATHS.items():
        p = _paths(FD, Dn, 33)
        assert (p["tiles"], p["nch"]) == (tiles, nch), (FD, Dn, p)
        assert p["split14"] == (len(tiles) == 14)
        seen_nch.add(nch)
        seen_tiles += tiles
    assert seen_nch == {1, 2, 3, 4, 5, 6, 7} and set(seen_tiles) == set("ESDPZ")
    # split14 with the three kinds of last tile (and a fourth: all dense)
    assert {LOADER_PATHS[s][0][-1] for s in ((416, 13), (432, 16), (448, 0))} == {"D", "S", "E"}
    # every shape at B = 33 and at one batch >= 255; 8 tiles = one full forward block, 9 = a second block with one wave
    by_shape = {}
    for FD, Dn, B, _, _ in MC.loader_cases():
        by_shape.setdefault((FD, Dn), set()).add(B)
    assert all(33 in bs and max(bs) >= 255 for bs in by_shape.values())
    assert set().union(*by_shape.values()) == {1, 31, 32, 33, 255, 256, 257}
    p8, p9 = _paths(64, 0, 256), _paths(64, 0, 257)
    assert (p8["ntiles"], p8["fwd_blocks"]) == (8, 1) and (p9["ntiles"], p9["fwd_blocks"]) == (9, 2)


@pytest.mark.parametrize("case", MC.loader_cases(),
                         ids=lambda c: f"FD{c[0]}Dn{c[1]}B{c[2]}H{'x'.join(map(str, c[3]))}{c[4]}")
def test_mlp_fwd_bwd_every_loader_against_float64(hip_lib, case):
    FD, Dn, B, hidden, act = case
    assert ops.mlp_supported(FD, Dn, list(hidden))
    p = _paths(FD, Dn, B)
    assert (p["tiles"], p["nch"]) == LOADER_PATHS[(FD, Dn)] and p["fwd_sweeps"] == p["bwd_sweeps"] == 1
    f, b = fwd_bwd(Case(FD, Dn, B, hidden, act))
    assert tuple(b.d_rows.v.shape) == (B, FD)


@pytest.mark.parametrize("case", MC.GRID_STRIDE_CASES, ids=lambda c: f"FD{c[0]}Dn{c[1]}B{c[2]}")
def test_mlp_fwd_bwd_grid_stride_against_float64(hip_lib, case):
    """(64, 3) at B = 2 * 256 * 32 + 17: the backward's 256 blocks take three tiles each (block 0) or two - the
    tile-ahead prefetch runs twice and then re-loads its own last tile.  (8, 0) at B = 65 536 + 33: the forward's
    256 blocks x 8 waves start a second sweep, of two tiles, the last one ragged."""
    FD, Dn, B, hidden, act = case
    p = _paths(FD, Dn, B)
    if FD == 64:
        assert p["ntiles"] == 513 and p["bwd_blocks"] == 256 and p["bwd_sweeps"] == 3 and B % 32 == 17
    else:
        assert p["ntiles"] == 2050 and p["fwd_blocks"] == 256 and p["fwd_sweeps"] == 2 and p["ntiles"] - 2048 == 2
    fwd_bwd(Case(FD, Dn, B, hidden, act))


# =============================================================================================== 2. the FM term
#            FD   Dn   D   form of g (S - E) in mlp_bwd_kernel
FM_CASES = [
    (64, 3, 16, "s_pf"),       # D = 16: S in registers
    (416, 13, 16, "s_pf"),     # ... at the Criteo shape, under split14
    (60, 4, 4, "lds"),         # the generic form: g * S staged in LDS
    (64, 0, 8, "lds"),
    (96, 0, 12, "lds"),        # D no power of two (k % D), with the zero-record padding tile
    (320, 64, 32, "lds"),      # D = 32 with Kp = 384
    (416, 13, 32, "global"),   # D = 32 with Kp = 448: past the LDS cap, g and S re-read from global memory
    (256, 33, 64, "global"),   # D = 64 with Kp = 320
    (448, 0, 64, "global"),    # D = 64 with Kp = 448, split14
    (192, 0, 64, "lds"),       # exactly the cap
]


@pytest.mark.parametrize("B", [33, 257])
@pytest.mark.parametrize("FD,Dn,D,form", FM_CASES, ids=lambda v: str(v))
def test_mlp_bwd_fm_term_three_forms_against_float64(hip_lib, FD, Dn, D, form, B):
    _cite("mlp.hip", "if (s_lds && !s_pf) {")
    _cite("mlp.hip", "const float4 s4 = *reinterpret_cast<const float4 *>(gS + row * D + (k % D));")
    _cite("mlp.hip", "const float4 s4 = *reinterpret_cast<const float4 *>(fm_sum + br * D + (k % D));")
    p = _paths(FD, Dn, B, D)
    assert p["fm"] == form and FD % D == 0
    if (FD, D) == (192, 64):
        assert _bwd_smem(192, 64) == LDS_CAP == p["smem"] == 163_840      # the launch asks for the whole LDS of a CU
    if form == "global":
        assert _bwd_smem(FD + Dn, D) > LDS_CAP and p["smem"] == _bwd_smem(FD + Dn, 0)
        assert (D >= 32 and p["Kp"] == 448) or (D == 64 and p["Kp"] >= 256)
    hidden, act = MC.HIDDEN[(FD // 4 + B) % 7], MC.ACTS[(D // 4 + B) % 3]
    c = Case(FD, Dn, B, hidden, act, D=D, seed=3)
    f, b = fwd_bwd(c)
    # the term is really there: without fm_sum the same call gives another d_rows
    b0 = Bwd(c, f.hv(), fm=False)
    check_bwd(c, f.hv(), b0, fm=False)
    assert not torch.equal(b0.d_rows.v, b.d_rows.v)


# ============================================================================================== 3. side outputs
@pytest.mark.parametrize("Dn", [1, 8, 31, 32])
def test_mlp_bwd_linear_term_gradients_against_float64(hip_lib, Dn):
    _cite("mlp.hip", "dxd += gv * xq[rc * xstride];")
    _cite("mlp.hip", "if (c < Dn) red[wave][kSgDense + c] = dxd;")
    _cite("mlp.hip", "const int sblk = (int)rm_grid_cap((ntiles + 3) / 4, 512);")
    for B in (33, 257):
        c = Case(32, Dn, B, (24, 32, 7), "leaky_relu", seed=4)
        f, b = fwd_bwd(c, xd_wsum=True, g_sum=True)
        R.assert_bits(b.dgs.v, b.dw0.v, "d_g_sum and d_w0_out are the same sum")
        only = Bwd(c, f.hv(), xd_wsum=True)       # d_g_sum NULL
        _same(b, only, f"Dn={Dn} B={B}: d_g_sum = NULL")


def test_mlp_bwd_rejects_d_xd_wsum_past_32_dense_columns(hip_lib):
    c = Case(32, 40, 33, (32,), "relu")
    f = Fwd(c)
    with pytest.raises(_lib.RecmanHipError, match="d_xd_wsum needs 1 <= Dn <= 32"):
        Bwd(c, f.hv(), xd_wsum=True)


def test_mlp_bwd_optional_outputs_streaming_reuse_and_determinism(hip_lib):
    _cite("mlp.hip", "if (flags & RM_MLP_STREAM_DROWS) {")
    c = Case(416, 13, 257, (32, 32), "relu", D=16, seed=5)
    f, b = fwd_bwd(c)
    for skip in ("db", "d_w_out", "d_w0_out"):
        o = Bwd(c, f.hv(), skip=(skip,))
        check_bwd(c, f.hv(), o)
        _same(b, o, f"{skip} = NULL")
    for what, kw in (("stream_d_rows", dict(stream=True)), ("the same call again", dict())):
        o = Bwd(c, f.hv(), **kw)
        check_bwd(c, f.hv(), o)      # (values, finiteness and the guard rows of every output, d_rows' among them)
        _same(b, o, what)
    # the same workspace, refilled with NaN, for a smaller batch: nothing of the larger call's partials is read
    c2 = Case(416, 13, 70, (32, 32), "relu", D=16, seed=6)
    f2 = Fwd(c2)
    check_fwd(c2, f2)
    b2 = Bwd(c2, f2.hv(), ws=b.ws)
    assert b2.ws.data_ptr() == b.ws.data_ptr()
    check_bwd(c2, f2.hv(), b2)


# ==================================================================================================== 4. the head
class Head:
    """The rm_mlp_tail of one case: guarded branch logits and labels in, guarded outputs."""

    def __init__(self, c, coefs, coef_mlp, task, ydt, grad_scale, skip=(), clip=False, seed=0):
        B = c.B
        gen = torch.Generator().manual_seed(100 + B + 7 * len(coefs) + seed)
        self.coefs, self.coef_mlp, self.task, self.grad_scale, self.skip = coefs, coef_mlp, task, grad_scale, skip
        br = [torch.randn(B, generator=gen) * 1.5 for _ in coefs]
        if clip:  # push |z| past 17 whatever the rest says (the caller asserts |rest| < 10)
            sign = torch.where(torch.rand(B, generator=gen) < 0.5, -1.0, 1.0)
            br[0] = sign * (30 + 10 * torch.rand(B, generator=gen)) / coefs[0]
            br[1:] = [t * 0.2 for t in br[1:]]
        self.branches = [(_in(t), co) for t, co in zip(br, coefs)]
        if task == "classification":
            y = (torch.rand(B, generator=gen) < 0.5)
            self.y = _in(y.to(ydt), BAD_LABEL if ydt == I64 else NAN)
        else:
            self.y = _in((torch.randn(B, generator=gen) * 2).to(ydt), NAN)
        self.ykw = dict(y=self.y) if ydt == I64 else dict(y_f=self.y)
        self.logit, self.pred, self.part, self.loss = _outs((B,), (B,), (cdiv(B, 32),), (1,))
        (self.dlogit,), self.dh = _outs((B,), fill=NAN), _outs(*[(B, 32)] * c.NL, fill=NAN)  # rm_mlp_bwd reads them
        opt = lambda name, a: None if name in skip else a.v
        self.tail = ops.mlp_tail(B, self.branches, coef_mlp, task=task, grad_scale=grad_scale,
                                 logit=opt("logit", self.logit), pred=opt("pred", self.pred), dlogit=self.dlogit.v,
                                 loss_partial=self.part.v, loss=opt("loss", self.loss), dh=[a.v for a in self.dh],
                                 **self.ykw)

    def outputs(self):
        o = dict(logit=self.logit, pred=self.pred, dlogit=self.dlogit, loss=self.loss)
        o.update({f"dh{l}": a for l, a in enumerate(self.dh)})
        return {k: v for k, v in o.items() if k not in self.skip}


def check_head(c, f, hd, what):
    """The head's outputs from the kernel's own dnn logit: logit inside the branch-sum bound (n = 3), pred / dlogit /
    loss at the transcendental tolerance, the loss and the gradient from the fp32 probabilities the kernel wrote."""
    B = c.B
    ref = M.head_ref(f.logit.v, hd.branches, hd.coef_mlp, hd.y, hd.task, hd.grad_scale)
    R.assert_within(hd.logit.v, ref["logit"], R.sum_bound(3, ref["logit_abs"]), f"{what}: logit", key="mlp_tail: logit")
    R.close(hd.pred.v, ref["pred"], what=f"{what}: pred")
    ref = M.head_ref(f.logit.v, hd.branches, hd.coef_mlp, hd.y, hd.task, hd.grad_scale, pred=hd.pred.v)
    R.close(hd.dlogit.v, ref["dlogit"], what=f"{what}: dlogit")
    R.close(hd.dlogit.v.double() * (B / hd.grad_scale), ref["dlogit"] * (B / hd.grad_scale), what=f"{what}: B * dlogit")
    R.close(hd.loss.v, ref["loss"], what=f"{what}: loss")
    for name, a in hd.outputs().items():
        a.check(f"{what}: {name}")
    hd.part.check(f"{what}: loss_partial")
    return ref


# coef_mlp is 1 throughout: dlogit is the MLP's own output gradient only then, and a tail takes no other value
# (include/recman_hip.h; the refusal has its test below)
HEAD_CASES = [  # B, hidden, act, branch coefficients, coef_mlp, task, label dtype, grad_scale
    (1, (32,), "relu", (), 1.0, "classification", I64, 1.0),
    (33, (32, 32), "relu", (1.0,), 1.0, "classification", I64, 0.25),
    (257, (24, 32, 7), "leaky_relu", (1.0, 1.0), 1.0, "classification", I64, 1.0),
    (257, (32, 1), "identity", (2.0, -0.5), 1.0, "regression", F32, 0.25),
    (33, (7, 32, 5), "leaky_relu", (-0.5,), 1.0, "classification", I64, 1.0),
    (33, (1,), "relu", (), 1.0, "regression", F32, 1.0),
    (1, (1, 1, 1), "identity", (2.0, 1.0), 1.0, "regression", F32, 0.25),
    (257, (32, 32), "relu", (-0.5, 2.0), 1.0, "classification", I64, 0.25),
]


def _head_run(c, hd):
    f = Fwd(c, tail=hd.tail)
    b = Bwd(c, f.hv(), g=hd.dlogit.v, tail=hd.tail, dh=hd.dh)
    return f, b


@pytest.mark.parametrize("B,hidden,act,coefs,coef_mlp,task,ydt,grad_scale", HEAD_CASES,
                         ids=lambda v: str(v).replace(" ", "").replace("torch.", ""))
def test_mlp_tail_against_float64_and_the_separate_kernels(hip_lib, B, hidden, act, coefs, coef_mlp, task, ydt,
                                                           grad_scale):
    _cite("mlp.hip", "if (tl.logit_a) z += tl.coef_a * ta; if (tl.logit_b) z += tl.coef_b * tb; z += tl.coef_mlp * dnn;")
    _cite("mlp.hip", "float gb = dz * (1.0f / (float)B); gb *= tl.grad_scale;")
    _cite("mlp.hip", "if (lane == 0) tl.loss_partial[tile] = ls;")
    _cite("mlp.hip", "if (!tail) {")   # the chain launch is skipped: dh comes from the forward's epilogue
    FD, Dn = (64, 3) if len(hidden) != 2 else (416, 13)
    c = Case(FD, Dn, B, hidden, act, D=16, seed=7)
    what = f"{c.what} head {coefs} {coef_mlp} {task} scale {grad_scale}"
    hd = Head(c, coefs, coef_mlp, task, ydt, grad_scale)
    f, b = _head_run(c, hd)
    check_fwd(c, f)
    check_head(c, f, hd, what)
    check_bwd(c, f.hv(), b)        # dh from the tail within the stage bounds of float64, and everything behind it
    # the chain kernel from the same g and h: bit for bit the tail's dh (and therefore the same gradients)
    plain = Bwd(c, f.hv(), g=hd.dlogit.v)
    check_bwd(c, f.hv(), plain)
    _same(b, plain, f"{what}: tail vs mlp_dh_chain_kernel")
    # rm_logit_loss on the same branches and the MLP's logit: the same arithmetic in the same order
    ll = dict(zip(("logit", "pred", "dlogit", "loss"), _outs((B,), (B,), (B,), (1,))))
    ops.logit_loss(hd.branches + [(f.logit.v, coef_mlp)], task=task, workspace=torch.full((1024,), NAN, device="cuda"),
                   **hd.ykw, **{k: a.v for k, a in ll.items()})
    R.assert_bits(hd.logit.v, ll["logit"].v, f"{what}: logit vs rm_logit_loss")
    R.assert_bits(hd.pred.v, ll["pred"].v, f"{what}: pred vs rm_logit_loss")
    R.assert_bits(hd.dlogit.v, ll["dlogit"].v * grad_scale, f"{what}: dlogit vs rm_logit_loss (grad_scale: a power of 2)")
    R.close(hd.loss.v, ll["loss"].v, what=f"{what}: loss vs rm_logit_loss")
    # each optional output NULL in turn: the others keep their bits
    for skip in ("logit", "pred", "loss"):
        h2 = Head(c, coefs, coef_mlp, task, ydt, grad_scale, skip=(skip,))
        f2, b2 = _head_run(c, h2)
        for k, a in h2.outputs().items():
            R.assert_bits(a.v, hd.outputs()[k].v, f"{what}: {k} with {skip} = NULL")
            a.check(f"{what}: {k} with {skip} = NULL")
        _untouched([getattr(h2, skip)], f"{what}: the {skip} arena nobody was given")
        R.assert_bits(f2.logit.v, f.logit.v, f"{what}: dnn logit with {skip} = NULL")
        _same(b, b2, f"{what}: gradients with {skip} = NULL")


@pytest.mark.parametrize("ydt", [I64, F32], ids=["int64", "float"])
def test_mlp_tail_clip_region_passes_no_gradient(hip_lib, ydt):
    """|z| > 17 for both labels: the probability lies outside [1e-7, 1 - 1e-7] (p = 1e-7 is |z| ~ 16.1), the clip
    passes no gradient - dlogit exactly 0, and with it every dh and every gradient of the backward."""
    B = 257
    c = Case(64, 3, B, (32, 32), "relu", D=16, seed=8)
    hd = Head(c, (1.0, 2.0), 1.0, "classification", ydt, 1.0, clip=True)
    f, b = _head_run(c, hd)
    check_fwd(c, f)
    assert float(f.logit.v.abs().max()) + float(hd.branches[1][0].abs().max()) * 2 < 10
    assert float(hd.logit.v.abs().min()) > 17
    y = hd.y.double()
    assert 0 < int(((hd.logit.v > 0) & (y > 0)).sum()) and 0 < int(((hd.logit.v > 0) & (y == 0)).sum())
    assert 0 < int(((hd.logit.v < 0) & (y > 0)).sum()) and 0 < int(((hd.logit.v < 0) & (y == 0)).sum())
    ref = check_head(c, f, hd, "clip region")
    assert torch.equal(ref["dlogit"], torch.zeros_like(ref["dlogit"]))
    R.assert_bits(hd.dlogit.v, torch.zeros(B, device="cuda"), "dlogit in the clip region")
    check_bwd(c, f.hv(), b)
    for l in range(c.NL):
        assert not bool(hd.dh[l].v.any()), f"dh{l} in the clip region"
    assert not bool(b.d_rows.v.any()) and not bool(b.dW[0].v.any())


# ========================================================================================== 5. rm_embed_mlp_fwd
EMF_LIN = {  # want_bias, want_lin, lin_w_dense, lin_w0: the four combinations the engines use, and all off
    "fm+lin+dense": (True, True, True, True), "lin+dense": (False, True, True, True),
    "fm+lin": (True, True, False, True), "lin": (False, True, False, True), "off": (False, False, False, False),
}
EMF_CASES = [  # F, Dn, table_ld, B, linear variant, hidden, act, outputs wanted (fm_sum, fm_logit, lin_logit), tail
    (1, 0, 32, 1, "fm+lin", (32,), "relu", (True, True, True), False),
    (1, 1, 20, 33, "fm+lin+dense", (7, 32, 5), "leaky_relu", (True, True, True), True),
    (2, 7, 32, 257, "lin+dense", (32, 32), "relu", (False, False, True), True),
    (3, 8, 20, 256, "fm+lin+dense", (24, 32, 7), "identity", (True, True, True), False),
    (4, 0, 32, 33, "lin", (32, 1), "relu", (True, False, True), True),
    (5, 9, 32, 257, "fm+lin+dense", (32, 32), "leaky_relu", (True, True, True), True),
    (26, 16, 32, 33, "fm+lin+dense", (32, 32), "relu", (True, True, True), True),
    (26, 1, 20, 256, "off", (1,), "relu", (False, False, False), False),
    (27, 16, 32, 257, "fm+lin+dense", (32, 32, 32), "relu", (True, True, True), True),
    (27, 0, 20, 33, "fm+lin", (1, 1, 1), "identity", (True, True, False), True),
    (3, 16, 32, 1, "off", (32, 32), "leaky_relu", (True, False, False), False),
]


class Front:
    """A fused table and ids that hit the first and the last row of every field and repeat; the fields' row ranges
    lie in the table in a shuffled order (field_off is not monotone)."""

    def __init__(self, F, ld, B, seed):
        gen = torch.Generator().manual_seed(seed)
        sizes = [3 + (5 * f) % 7 for f in range(F)]
        order = list(range(1, F, 2)) + list(range(0, F, 2))
        off, at = [0] * F, 0
        for f in order:
            off[f], at = at, at + sizes[f]
        assert F < 2 or off != sorted(off)
        idx = torch.stack([torch.randint(0, s, (B,), generator=gen) for s in sizes], 1)
        idx[0] = 0
        idx[-1] = torch.tensor(sizes) - 1
        if B > 2:
            idx[B // 2] = idx[0] if B < 5 else idx[1]     # a repeated row of ids
        self.table = _in(torch.randn(at, ld, generator=gen) * 0.3)
        self.idx = _in(idx, BAD_ID)
        self.off = torch.tensor(off, dtype=I64, device="cuda")
        self.R = at


@pytest.mark.parametrize("F,Dn,ld,B,lin,hidden,act,want,tail", EMF_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_embed_mlp_fwd_against_float64(hip_lib, F, Dn, ld, B, lin, hidden, act, want, tail):
    _embed_mlp_fwd_case(F, Dn, ld, B, lin, hidden, act, want, tail)


def _embed_mlp_fwd_case(F, Dn, ld, B, lin, hidden, act, want, tail):
    _cite("mlp.hip", "const int nhc = Kp / 32;")
    _cite("mlp.hip", "const int nf = F - 2 * hc;")      # odd F: a half chunk with one live field
    _cite("mlp.hip", "const float *p = ef.table + rows[q] * ef.table_ld + sub * 4;")
    assert ops.embed_mlp_fwd_supported(F, 16, ld, Dn, list(hidden))
    FD = 16 * F
    assert _kp(FD + Dn) <= 448 and ((F, Dn) != (27, 16) or FD + Dn == 448)
    want_bias, want_lin, has_wd, has_w0 = EMF_LIN[lin]
    has_wd = has_wd and Dn > 0
    c = Case(FD, Dn, B, hidden, act, D=16, seed=9)      # its xe is not used: E comes from the gather
    fr = Front(F, ld, B, seed=F + Dn)
    gen = torch.Generator().manual_seed(F)
    wd = (torch.randn(Dn, generator=gen) * 0.5).cuda() if has_wd else None
    lw0 = torch.randn(1, generator=gen).cuda() if has_w0 else None
    flat = fr.table.reshape(-1)
    ref = R.embed_fwd_ref(fr.idx, fr.table, fr.off, 16, bias=flat[16:] if want_bias else None, bias_ld=ld,
                          lin=flat[17:] if want_lin else None, lin_ld=ld, lin_off=fr.off, lin_w_dense=wd, lin_w0=lw0,
                          dense=c.xd if has_wd else None)
    what = f"embed_mlp_fwd F={F} Dn={Dn} ld={ld} B={B} {lin}"

    def run(stream_rows, with_tail):
        E, S, fml, linl = _outs((B, F, 16), (B, 16), (B,), (B,), fill=NAN)   # xe, fm_sum and branches of what follows
        f = Fwd(c, run=False)
        hd = None
        if with_tail:
            hd = Head(c, (1.0, 1.0), 1.0, "classification", I64, 1.0)
            # the head's other branches are this call's own lin_logit / fm_logit buffers (or absent)
            br = [a.v for a, w in ((linl, want[2]), (fml, want[1])) if w]
            hd.branches = [(t, 1.0) for t in br]
            hd.tail = ops.mlp_tail(B, hd.branches, 1.0, y=hd.y, logit=hd.logit.v, pred=hd.pred.v, dlogit=hd.dlogit.v,
                                   loss_partial=hd.part.v, loss=hd.loss.v, dh=[a.v for a in hd.dh])
        ops.embed_mlp_fwd(fr.idx, fr.table, fr.off, 16, ld, c.xd, c.Ws, c.bs, c.w_out, c.w0, act, E.v, f.hv(),
                          f.logit.v, want_bias=want_bias, want_lin=want_lin, lin_w_dense=wd, lin_w0=lw0,
                          fm_sum=S.v if want[0] else None, fm_logit=fml.v if want[1] else None,
                          lin_logit=linl.v if want[2] else None, stream_rows=stream_rows,
                          tail=None if hd is None else hd.tail)
        return dict(E=E, fm_sum=S, fm_logit=fml, lin_logit=linl), f, hd

    o, f, hd = run(False, tail)
    R.assert_bits(o["E"].v, ref["E"], f"{what}: E")
    if want[0]:
        R.assert_within(o["fm_sum"].v, ref["fm_sum"], R.sum_bound(F, ref["fm_sum_abs"]), f"{what}: fm_sum",
                        key="embed_mlp_fwd: fm_sum")                                            # n = F
    if want[1]:
        R.assert_within(o["fm_logit"].v, ref["fm_logit"], ref["fm_logit_bound"], f"{what}: fm_logit",
                        key="embed_mlp_fwd: fm_logit")
    if want[2]:
        R.assert_within(o["lin_logit"].v, ref["lin_logit"], R.sum_bound(ref["lin_n"], ref["lin_abs"]),
                        f"{what}: lin_logit", key="embed_mlp_fwd: lin_logit")                   # n = F + Dn + 1
    for k, a in o.items():
        a.check(f"{what}: {k}")   # an output that was not wanted keeps its sentinel everywhere
        if not dict(E=True, fm_sum=want[0], fm_logit=want[1], lin_logit=want[2])[k]:
            R.assert_bits(a.v, torch.full_like(a.v, a.fill), f"{what}: {k} was not asked for")
    # the MLP on x = [E | xd], E the kernel's own (bit-checked) output
    c.xe = o["E"].v.reshape(B, FD)
    c.x = c.xe if c.xd is None else torch.cat([c.xe, c.xd], 1)
    check_fwd(c, f, key="embed_mlp_fwd")
    if tail:
        c.S = o["fm_sum"].v if want[0] else None
        b = Bwd(c, f.hv(), g=hd.dlogit.v, tail=hd.tail, dh=hd.dh)   # (its finishing kernel reduces the head's loss)
        check_head(c, f, hd, what)
        check_bwd(c, f.hv(), b, fm=want[0])
    # streamed row loads: the same bits everywhere
    o2, f2, hd2 = run(True, tail)
    for k in o:
        R.assert_bits(o2[k].v, o[k].v, f"{what}: {k} with stream_rows")
    for l in range(c.NL):
        R.assert_bits(f2.h[l].v, f.h[l].v, f"{what}: h{l} with stream_rows")
    R.assert_bits(f2.logit.v, f.logit.v, f"{what}: logit with stream_rows")
    if tail:
        for k, a in hd.outputs().items():
            if k != "loss":   # (the loss is reduced by the backward's finishing kernel, not run a second time)
                R.assert_bits(hd2.outputs()[k].v, a.v, f"{what}: head {k} with stream_rows")
    # with a tail and without: the forward's own outputs do not depend on it
    o3, f3, _ = run(False, not tail)
    R.assert_bits(f3.logit.v, f.logit.v, f"{what}: logit with{'out' if tail else ''} a tail")
    R.assert_bits(o3["E"].v, o["E"].v, f"{what}: E with{'out' if tail else ''} a tail")
    return dict({k: a.v for k, a in o.items()}, h=f.hv(), logit=f.logit.v)


# ============================================================================================ 6. argument checks
def _untouched(arenas, what):
    for a in arenas:
        R.assert_bits(a.full, torch.full_like(a.full, a.fill), f"{what}: an output was written")


def _raw_case(FD, Dn, B, hidden):
    """Tensors of the right shapes for a call that must be refused before anything is launched."""
    dims = [FD + Dn] + list(hidden)
    z = lambda *s: torch.zeros(*s, device="cuda")
    return dict(xe=z(B, FD), xd=z(B, Dn) if Dn else None, Ws=[z(dims[l], dims[l + 1]) for l in range(len(hidden))],
                bs=[z(h) for h in hidden], w_out=z(hidden[-1]), w0=z(1))


@pytest.mark.parametrize("FD,Dn,hidden,msg", [
    (32, 3, (33,), "hidden width 33 unsupported"),
    (32, 3, (8, 8, 8, 8), "4 hidden layers unsupported"),
    (30, 3, (8,), "input width 30\\+3 unsupported"),
    (448, 1, (8,), "input width 448\\+1 unsupported"),
], ids=["H33", "NL4", "FD%4", "K449"])
def test_mlp_entry_points_refuse_unsupported_shapes_and_launch_nothing(hip_lib, FD, Dn, hidden, msg):
    B = 33
    assert not ops.mlp_supported(FD, Dn, list(hidden))
    p = _raw_case(FD, Dn, B, hidden)
    h, (logit, d_rows) = _outs(*[(B, 32)] * len(hidden)), _outs((B,), (B, FD))
    with pytest.raises(_lib.RecmanHipError, match=msg):
        ops.mlp_fwd(p["xe"], p["xd"], p["Ws"], p["bs"], p["w_out"], p["w0"], "relu", [a.v for a in h], logit.v)
    dh, dW = _outs(*[(B, 32)] * len(hidden)), _outs(*[tuple(W.shape) for W in p["Ws"]])
    ws = torch.full((ops.mlp_bwd_workspace(FD, Dn),), SENT, device="cuda")
    with pytest.raises(_lib.RecmanHipError, match=msg):
        ops.mlp_bwd(p["xe"], p["xd"], p["Ws"], p["w_out"], "relu", torch.zeros(B, device="cuda"),
                    [torch.zeros(B, 32, device="cuda") for _ in hidden], d_rows.v, [a.v for a in dh],
                    [a.v for a in dW], ws)
    torch.cuda.synchronize()
    _untouched(h + [logit, d_rows] + dh + dW, msg)
    assert bool((ws == SENT).all())


def test_mlp_tail_needs_exactly_one_kind_of_label(hip_lib):
    B = 33
    c = Case(32, 3, B, (8,), "relu")
    y, y_f = torch.zeros(B, dtype=I64, device="cuda"), torch.zeros(B, device="cuda")
    outs = _outs((B,), (cdiv(B, 32),), (B, 32))
    kw = dict(dlogit=outs[0].v, loss_partial=outs[1].v, dh=[outs[2].v])
    for labels in (dict(), dict(y=y, y_f=y_f)):
        with pytest.raises(ValueError, match="exactly one of y / y_f"):
            ops.mlp_tail(B, [], 1.0, **labels, **kw)
    # ... and the library refuses a struct that reaches it in that state
    for both in (True, False):
        t = ops.mlp_tail(B, [], 1.0, y=y, **kw)
        if both:
            t.y_f = y_f.data_ptr()
        else:
            t.y = None
        f = Fwd(c, run=False)
        with pytest.raises(_lib.RecmanHipError, match="tail needs exactly one of y / y_f"):
            ops.mlp_fwd(c.xe, c.xd, c.Ws, c.bs, c.w_out, c.w0, "relu", f.hv(), f.logit.v, tail=t)
        torch.cuda.synchronize()
        _untouched(f.h + [f.logit] + outs, "tail with both or neither label")


@pytest.mark.parametrize("coef", [2.0, -0.5])
def test_mlp_tail_refuses_a_scaled_mlp_logit(hip_lib, coef):
    """final logit = coef_mlp dnn + ..., so dLoss/d(dnn) = coef_mlp dlogit: the tail's dh chain and rm_mlp_bwd's
    d_w_out / d_w0_out, which take dlogit itself, are the gradients only for coef_mlp = 1.  The wrapper and all three
    entry points refuse anything else and launch nothing."""
    _cite("mlp.hip", 'RM_REQUIRE(t->coef_mlp == 1.0f, "%s: tail coef_mlp must be 1 (got %g)", fn, (double)t->coef_mlp);')
    B, F, Dn = 33, 2, 3
    c = Case(16 * F, Dn, B, (8,), "relu", D=16)
    y = torch.zeros(B, dtype=I64, device="cuda")
    dlogit, part, dh = _outs((B,), (cdiv(B, 32),), (B, 32))
    kw = dict(y=y, dlogit=dlogit.v, loss_partial=part.v, dh=[dh.v])
    with pytest.raises(ValueError, match="coef_mlp must be 1"):
        ops.mlp_tail(B, [], coef, **kw)
    t = ops.mlp_tail(B, [], 1.0, **kw)
    t.coef_mlp = coef      # a struct that reaches the library in that state
    f = Fwd(c, run=False)
    with pytest.raises(_lib.RecmanHipError, match="rm_mlp_fwd: tail coef_mlp must be 1"):
        ops.mlp_fwd(c.xe, c.xd, c.Ws, c.bs, c.w_out, c.w0, "relu", f.hv(), f.logit.v, tail=t)
    fr = Front(F, 32, B, seed=1)
    (E,) = _outs((B, F, 16))
    with pytest.raises(_lib.RecmanHipError, match="rm_embed_mlp_fwd: tail coef_mlp must be 1"):
        ops.embed_mlp_fwd(fr.idx, fr.table, fr.off, 16, 32, c.xd, c.Ws, c.bs, c.w_out, c.w0, "relu", E.v, f.hv(),
                          f.logit.v, tail=t)
    d_rows, dW = _outs((B, c.FD), tuple(c.Ws[0].shape))
    ws = torch.full((ops.mlp_bwd_workspace(c.FD, Dn),), SENT, device="cuda")
    with pytest.raises(_lib.RecmanHipError, match="rm_mlp_bwd: tail coef_mlp must be 1"):
        ops.mlp_bwd(c.xe, c.xd, c.Ws, c.w_out, "relu", c.g, [torch.zeros(B, 32, device="cuda")], d_rows.v, [dh.v],
                    [dW.v], ws, tail=t)
    torch.cuda.synchronize()
    _untouched(f.h + [f.logit, E, dlogit, part, dh, d_rows, dW], "tail with coef_mlp != 1")
    assert bool((ws == SENT).all())


def test_embed_mlp_fwd_refuses_a_foreign_branch_in_its_tail(hip_lib):
    B, F, Dn = 33, 2, 3
    c = Case(16 * F, Dn, B, (8,), "relu")
    fr = Front(F, 32, B, seed=1)
    E, S, fml, linl, dlogit, part, dh = _outs((B, F, 16), (B, 16), (B,), (B,), (B,), (cdiv(B, 32),), (B, 32))
    foreign = torch.zeros(B, device="cuda")
    t = ops.mlp_tail(B, [(foreign, 1.0)], 1.0, y=torch.zeros(B, dtype=I64, device="cuda"), dlogit=dlogit.v,
                     loss_partial=part.v, dh=[dh.v])
    f = Fwd(c, run=False)
    with pytest.raises(_lib.RecmanHipError, match="must be this call's lin_logit / fm_logit buffers"):
        ops.embed_mlp_fwd(fr.idx, fr.table, fr.off, 16, 32, c.xd, c.Ws, c.bs, c.w_out, c.w0, "relu", E.v, f.hv(),
                          f.logit.v, want_bias=True, want_lin=True, fm_sum=S.v, fm_logit=fml.v, lin_logit=linl.v,
                          tail=t)
    torch.cuda.synchronize()
    _untouched([E, S, fml, linl, dlogit, part, dh, f.logit] + f.h, "foreign tail branch")


# ======================================================================================================= the table
RATIO_KEYS = ("mlp_fwd: h", "mlp_fwd: logit", "mlp_bwd: dh", "mlp_bwd: d_rows", "mlp_bwd: dW0", "mlp_bwd: dW_l",
              "mlp_bwd: db", "mlp_bwd: d_w_out", "mlp_bwd: sum g", "mlp_bwd: d_xd_wsum", "mlp_tail: logit",
              "embed_mlp_fwd: h", "embed_mlp_fwd: logit", "embed_mlp_fwd: fm_sum", "embed_mlp_fwd: fm_logit",
              "embed_mlp_fwd: lin_logit")


def test_zz_report_error_to_bound_ratios(hip_lib):
    """Largest |error| / bound per kernel over every check this module made (runs last; nothing is tuned to it)."""
    keys = sorted(k for k in R.RATIOS if k.split(":")[0] in ("mlp_fwd", "mlp_bwd", "mlp_tail", "embed_mlp_fwd"))
    missing = set(RATIO_KEYS) - set(keys)
    assert not missing, f"no check recorded {sorted(missing)}: this table reports the WHOLE module, run it as a whole"
    print("\nerr / bound, largest over the module:")
    for k in keys:
        print(f"  {k:32s} {R.RATIOS[k]:.3f}")
    assert all(R.RATIOS[k] <= 1.0 for k in keys)
