"""GPU: the small kernels every model runs before and after the big ones - csrc/embed.hip, loss.hip, pool.hip,
route.hip and dense_opt_kernel of optim.hip - called through their recman_amd/ops.py wrappers and compared with the
float64 references of tests/front_refs.py, at the shapes where such kernels go wrong: field-chunk edges, every group
width the gather dispatches, second and third grid-stride sweeps with ragged tails, the router's multi-chunk blocks,
the three paths of the column sums, element offsets beyond 2^31.

How each output is compared is fixed by its arithmetic (tests/front_refs.py): data movement and single fp32
operations bit for bit; sums of n products within (n + 2) 2^-24 sum|terms| of float64 (the n is stated at every
call); outputs that pass through expf / logf / rsqrtf at rtol 1e-5, atol 1e-6.  No example or element is left out of
any comparison.  Every case that claims to reach a path restates the launch arithmetic of the C++ it cites
(`_cite` fails when that source text changes, the asserts when the numbers do).

The largest error / bound ratio seen per kernel is collected in front_refs.RATIOS and printed by the last test."""
import os

import pytest
import torch

from recman_amd import _lib, ops
from recman_amd.dist import route_torch
from tests import front_refs as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, I64 = torch.float32, torch.float64, torch.int64
KBLOCK = 256


def cdiv(a, b):
    return -(-a // b)


_SRC = {}


def _cite(name, snippet):
    """The launch code a case relies on, as it stands in recman_amd/csrc/<name> (whitespace-insensitive)."""
    if name not in _SRC:
        with open(os.path.join(ROOT, "recman_amd", "csrc", name)) as f:
            _SRC[name] = " ".join(f.read().split())
    assert " ".join(snippet.split()) in _SRC[name], f"csrc/{name} no longer contains `{snippet}`: re-derive this case"


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device="cuda", dtype=F32)


def _randint(g, hi, *shape):
    return torch.randint(0, hi, shape, generator=g, device="cuda", dtype=I64)


def _keep_mask(g, *shape):
    """FMLayer dropout multipliers at keep 0.8: 0 or 1 / 0.8."""
    return (torch.rand(*shape, generator=g, device="cuda") < 0.8).float() / 0.8


def _sentinel(*shape, value=-777.25):
    return torch.full(shape, value, device="cuda", dtype=F32)


# =================================================================================================================
# 1. embedding forward (rm_embed_fwd)
EMBED_GRID_CAP = 256 * 16   # blocks
UNFUSED_CHUNK, FUSED_CHUNK = 8, 13
UNFUSED_F = (1, 7, 8, 9, 17)
FUSED_F = (1, 12, 13, 14, 26, 27, 40)
ALL_D = (4, 8, 16, 32, 64, 128, 256)
LAYOUTS = ("sep", "strided13", "strided31", "fused", "fused_bias", "fused_lin")


def _cite_embed_launch():
    _cite("embed.hip", "constexpr int kUnroll = 8;")
    _cite("embed.hip", "#define RM_FUSED_UNROLL 13")
    _cite("embed.hip", "const int epw = 64 / G; const int64_t waves = (B + epw - 1) / epw; "
                       "dim3 grid(rm_grid_cap((waves + 3) / 4, 256 * 16));")
    _cite("embed.hip", "const int GF = (int)table_ld / 4; const int epwf = 64 / GF; "
                       "const int64_t wavesf = (B + epwf - 1) / epwf; dim3 gridf(rm_grid_cap((wavesf + 3) / 4, 256 * 16));")
    _cite("embed.hip", "for (int64_t b0 = wave * EPW; b0 < B; b0 += nwaves * EPW)")
    # the dispatch: csrc/embed.hip, rm_embed_fwd, "fused-row layout"
    _cite("embed.hip", "const bool pow2 = table_ld >= D + 4 && table_ld <= 256 && (table_ld & (table_ld - 1)) == 0;")
    _cite("embed.hip", "if (pow2 && bias_in_row && lin_in_row && table_ld == 2 * D && (bias_table || lin_w))")


def _runs_fused(D, table_ld, bias_in_row, lin_in_row, has_bias, has_lin):
    """The dispatch condition of rm_embed_fwd restated (csrc/embed.hip, "fused-row layout")."""
    pow2 = D + 4 <= table_ld <= 256 and table_ld & (table_ld - 1) == 0
    return pow2 and bias_in_row and lin_in_row and table_ld == 2 * D and (has_bias or has_lin)


def _epw(D, fused):
    return 64 // ((2 * D if fused else D) // 4)


def _sweep(D, fused):
    """Examples one pass of the capped grid covers: 256 * 16 blocks of 4 waves of EPW examples."""
    return EMBED_GRID_CAP * 4 * _epw(D, fused)


class EmbedCase:
    """Tables, ids and side inputs of one rm_embed_fwd call, with the wrapper's and the reference's arguments."""

    def __init__(self, B, F, D, layout, seed, mask_b=False, mask_e=False, Dn=13, w0=True, reuse=False):
        g = _gen(seed)
        self.B, self.F, self.D, self.layout = B, F, D, layout
        sizes = torch.tensor([3 + (7 * f) % 11 for f in range(F)], device="cuda")
        self.field_off = (torch.cumsum(sizes, 0) - sizes).contiguous()
        Rn = int(sizes.sum())
        idx = (torch.rand(B, F, generator=g, device="cuda") * sizes).long().clamp(max=sizes - 1)
        idx[0] = sizes - 1          # every field's last row ...
        if B > 1:
            idx[1] = 0              # ... and its row 0: a wrong field_off[f] for a clamped f changes a value
        if reuse:                   # Zipf's limit: every example asks for the same row of these fields
            idx[:, 0], idx[:, F - 1] = sizes[0] - 1, 0
        self.idx = idx.contiguous()
        fused = layout.startswith("fused")
        ld = 2 * D if fused else D + 20 if layout.startswith("strided") else D
        self.table = _randn(g, Rn, ld)
        self.kw = dict(table_ld=ld, D=D)
        self.ref_kw = {}
        has_bias, has_lin = layout != "fused_lin", layout != "fused_bias"
        if fused:
            flat = self.table.reshape(-1)
            if has_bias:
                self.kw["bias_col"] = D
                self.ref_kw.update(bias=flat[D:], bias_ld=ld)
            if has_lin:
                self.kw["lin_col"] = D + 1
                self.ref_kw.update(lin=flat[D + 1:], lin_ld=ld, lin_off=self.field_off)
        else:
            bl, ll = {"sep": (1, 1), "strided13": (1, 3), "strided31": (3, 1)}[layout]
            self.bias_t = _randn(g, Rn * bl)
            self.lin_off = (self.field_off + 5).contiguous()   # the linear blocks start behind 5 other weights
            self.lin_t = _randn(g, (Rn + 5) * ll)
            self.kw.update(bias_table=self.bias_t, bias_ld=bl, lin_w=self.lin_t, lin_ld=ll, lin_off=self.lin_off)
            self.ref_kw.update(bias=self.bias_t, bias_ld=bl, lin=self.lin_t, lin_ld=ll, lin_off=self.lin_off)
        self.fused = _runs_fused(D, ld, fused, fused, has_bias, has_lin)
        if Dn:
            self.dense, self.lin_w_dense = _randn(g, B, Dn), _randn(g, Dn)
            self.kw.update(dense=self.dense, lin_w_dense=self.lin_w_dense)
            self.ref_kw.update(dense=self.dense, lin_w_dense=self.lin_w_dense)
        if w0:
            self.lin_w0 = _randn(g, 1)
            self.kw["lin_w0"] = self.ref_kw["lin_w0"] = self.lin_w0
        if mask_b:
            self.kw["mask_b"] = self.ref_kw["mask_b"] = _keep_mask(g, B, F)
        if mask_e:
            self.kw["mask_e"] = self.ref_kw["mask_e"] = _keep_mask(g, B, F, D)

    def outputs(self):
        B, F, D = self.B, self.F, self.D
        return dict(E=_sentinel(B, F, D), fm_sum=_sentinel(B, D), fm_logit=_sentinel(B), lin_logit=_sentinel(B))

    def run(self, stream_rows=False, skip=()):
        out = {k: v for k, v in self.outputs().items() if k not in skip}
        ops.embed_fwd(self.idx, self.table, self.field_off, stream_rows=stream_rows, **self.kw, **out)
        return out

    def check(self, out, what):
        """All four outputs at EVERY example: E bit for bit; fm_sum n = F; fm_logit the nested bound of
        tests/front_refs.py; lin_logit n = F + Dn + 1."""
        ref = R.embed_fwd_ref(self.idx, self.table, self.field_off, self.D, **self.ref_kw)
        fam = "embed_fwd fused" if self.fused else "embed_fwd unfused"
        if "E" in out:
            R.assert_bits(out["E"], ref["E"], f"{what}: E")
        if "fm_sum" in out:
            R.assert_within(out["fm_sum"], ref["fm_sum"], R.sum_bound(self.F, ref["fm_sum_abs"]), f"{what}: fm_sum",
                            key=f"{fam}: fm_sum")
        if "fm_logit" in out:
            R.assert_within(out["fm_logit"], ref["fm_logit"], ref["fm_logit_bound"], f"{what}: fm_logit",
                            key=f"{fam}: fm_logit")
        if "lin_logit" in out:
            R.assert_within(out["lin_logit"], ref["lin_logit"], R.sum_bound(ref["lin_n"], ref["lin_abs"]),
                            f"{what}: lin_logit", key=f"{fam}: lin_logit")


def _embed_variants(fused):
    """(mask_b, mask_e, stream_rows): unmasked, masked both ways; the non-temporal kernel exists for fused rows."""
    v = [(False, False, False), (True, True, False)]
    return v + [(False, False, True)] if fused else v


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("D", ALL_D)
def test_embed_fwd_every_width_and_layout(hip_lib, D, layout):
    """Every D the dispatch takes (G = D / 4 = 1 .. 64 lanes per example; fused GF = 2 .. 64) with every table layout,
    masked and unmasked (and non-temporal where the fused kernel runs), F walking the chunk-edge list of the kernel
    that runs.  D = 256 in a fused row has table_ld = 512 > 256: outside the fused kernel, answered by the unfused one."""
    _cite_embed_launch()
    i = ALL_D.index(D) + LAYOUTS.index(layout)
    want_fused = layout.startswith("fused") and D <= 128
    Fs = FUSED_F if want_fused else UNFUSED_F
    for j, (mb, me, nt) in enumerate(_embed_variants(want_fused)):
        F = Fs[(i + j) % len(Fs)]
        c = EmbedCase(255, F, D, layout, seed=100 * D + i + j, mask_b=mb, mask_e=me)
        assert c.fused == want_fused, (D, layout)
        c.check(c.run(stream_rows=nt), f"D={D} {layout} F={F} masks={mb, me} nt={nt}")


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_embed_fwd_field_chunk_edges_and_small_batches(hip_lib, fused):
    """F across the edges of the field chunks (8 unfused: 7/8/9, 16/17; 13 fused: 12/13/14, 26/27, 39/40 - the last
    chunk clamps f to F - 1) x B around one wave's examples, for every kernel variant; D = 16 (EPW 16 resp. 8)."""
    _cite_embed_launch()
    _cite("embed.hip", "const int f = f0 + u < F ? f0 + u : F - 1;")
    D, layout = 16, "fused" if fused else "sep"
    epw = _epw(D, fused)
    assert epw == (8 if fused else 16)
    Fs = FUSED_F if fused else UNFUSED_F
    chunk = FUSED_CHUNK if fused else UNFUSED_CHUNK
    assert {chunk - 1, chunk, chunk + 1, 2 * chunk + 1} <= set(Fs) and 1 in Fs
    masks = [(False, False, False), (True, False, False), (False, True, False), (True, True, False)]
    for F in Fs:
        for B in (1, 2, epw - 1, epw + 1, 255):
            for mb, me, nt in masks + ([(False, False, True)] if fused else []):
                c = EmbedCase(B, F, D, layout, seed=F * 1000 + B, mask_b=mb, mask_e=me)
                assert c.fused == fused
                c.check(c.run(stream_rows=nt), f"{layout} F={F} B={B} masks={mb, me} nt={nt}")


SWEEP_CASES = [("sep", 64, 9), ("fused", 32, 14), ("fused", 128, 27)]


SWEEP_PARAMS = [(l, D, F, v) for l, D, F in SWEEP_CASES for v in ("plain", "masked", "reuse", "nt")
                if v != "nt" or l == "fused"]   # (the non-temporal kernel exists for fused rows only)


@pytest.mark.parametrize("layout,D,F,variant", SWEEP_PARAMS, ids=lambda v: str(v))
def test_embed_fwd_third_sweep_with_ragged_tail(hip_lib, layout, D, F, variant):
    """B = 2 sweeps + an odd remainder: every wave runs its grid-stride loop twice, some a third time, and the last
    wave is ragged; F sits one past a chunk edge.  `reuse`: every example asks for the same row of two fields."""
    _cite_embed_launch()
    fused = layout == "fused"
    sweep = _sweep(D, fused)
    assert sweep == {("sep", 64): 65536, ("fused", 32): 65536, ("fused", 128): 16384}[(layout, D)]
    B = 2 * sweep + 37
    epw = _epw(D, fused)
    waves = cdiv(B, epw)
    assert cdiv(waves, 4) > EMBED_GRID_CAP                  # the grid is capped ...
    assert 2 * sweep < B < 3 * sweep and (B % epw != 0 or epw == 1) and waves % 4 != 0   # ... a third, ragged pass
    assert F % (FUSED_CHUNK if fused else UNFUSED_CHUNK) == 1
    m = variant == "masked"
    c = EmbedCase(B, F, D, layout, seed=D + F, mask_b=m, mask_e=m, reuse=variant == "reuse")
    assert c.fused == fused
    c.check(c.run(stream_rows=variant == "nt"), f"{layout} D={D} B={B} {variant}")


@pytest.mark.parametrize("layout,D,F", [("sep", 16, 9), ("strided31", 8, 17), ("fused", 16, 14), ("fused", 64, 27)])
def test_embed_fwd_optional_arguments(hip_lib, layout, D, F):
    """Non-temporal loads bit-equal to the plain ones; each output pointer NULL in turn leaves the others
    bit-identical; Dn in {0, 1, 13}; lin_w0 NULL."""
    for Dn, w0 in ((13, True), (1, True), (0, True), (13, False), (0, False)):
        c = EmbedCase(301, F, D, layout, seed=7 * D + Dn, Dn=Dn, w0=w0)
        full = c.run()
        c.check(full, f"{layout} D={D} Dn={Dn} w0={w0}")
        nt = c.run(stream_rows=True)
        for k in full:
            R.assert_bits(nt[k], full[k], f"RM_EMBED_STREAM_ROWS: {k}")
        for skip in full:
            part = c.run(skip=(skip,))
            assert skip not in part
            for k in part:
                R.assert_bits(part[k], full[k], f"{k} with {skip} = NULL")


def test_embed_fwd_rejects_what_it_does_not_take(hip_lib):
    """Negative return (the wrapper raises) with the argument named in rm_last_error."""
    c = EmbedCase(8, 3, 16, "sep", seed=1)
    idx, fo = c.idx, c.field_off
    for D in (12, 512):
        t = _randn(_gen(2), int(fo[-1]) + 20, D)
        with pytest.raises(_lib.RecmanHipError, match=f"D={D} unsupported"):
            ops.embed_fwd(idx, t, fo, E=torch.empty(8, 3, D, device="cuda"))
    buf = torch.empty(8 * 3 * 16 + 4, device="cuda")
    E_off = buf[1:1 + 8 * 3 * 16].view(8, 3, 16)
    assert E_off.data_ptr() % 16 == 4
    with pytest.raises(_lib.RecmanHipError, match="E must be 16-byte aligned"):
        ops.embed_fwd(idx, c.table, fo, E=E_off)
    t18 = _randn(_gen(3), c.table.shape[0], 18)
    with pytest.raises(_lib.RecmanHipError, match=r"ld % 4 == 0 \(ld=18\)"):
        ops.embed_fwd(idx, t18, fo, table_ld=18, D=16, E=torch.empty(8, 3, 16, device="cuda"))


# =================================================================================================================
# 2. embedding backward, scatter, linear term
ELEMENTWISE_THREADS = 256 * 16 * KBLOCK   # rm_grid_cap(.., 256 * 16) blocks of 256 threads: one sweep


def _cite_elementwise(name, entry_total):
    _cite(name, entry_total)
    assert ELEMENTWISE_THREADS == 1_048_576


@pytest.mark.parametrize("B,F,D", [(1, 1, 4), (255, 5, 12), (70_001, 5, 32)])
def test_embed_bwd_against_float64(hip_lib, B, F, D):
    """d_rows within the n = 6 bound (front_refs.EMBED_BWD_N), d_bias one fp32 product: bit for bit.  With and
    without g_fm, dE_up NULL, d_rows aliasing dE_up, masks, D = 12 (any multiple of 4).  g_fm NULL: d_rows is dE_up's
    bits and d_bias is left untouched (include/recman_hip.h says so; pinned with a sentinel)."""
    _cite_elementwise("embed.hip", "const int64_t total = B * F * G; dim3 grid(rm_grid_cap((total + kBlock - 1) / kBlock, 256 * 16));")
    total = B * F * D // 4
    if B == 70_001:   # a third sweep, ragged to the thread: 2 800 040 float4 over 1 048 576 threads
        assert total == 2_800_040 > 2 * ELEMENTWISE_THREADS and total % ELEMENTWISE_THREADS % KBLOCK != 0
    g = _gen(B + D)
    E, dE_up, g_fm = _randn(g, B, F, D), _randn(g, B, F, D), _randn(g, B)
    for mb, me in ((False, False), (True, True), (False, True), (True, False)):
        mask_b = _keep_mask(g, B, F) if mb else None
        mask_e = _keep_mask(g, B, F, D) if me else None
        m = E if mask_e is None else E * mask_e
        fm_sum = m.double().sum(1).float()
        for up in (dE_up, None):
            want, ab, want_bias = R.embed_bwd_ref(E, fm_sum, up, g_fm, mask_b, mask_e)
            d_rows, d_bias = _sentinel(B, F, D), _sentinel(B, F)
            ops.embed_bwd(d_rows, E=E, fm_sum=fm_sum, dE_up=up, g_fm=g_fm, mask_b=mask_b, mask_e=mask_e, d_bias=d_bias)
            what = f"embed_bwd B={B} masks={mb, me} dE_up={'yes' if up is not None else 'NULL'}"
            R.assert_within(d_rows, want, R.sum_bound(R.EMBED_BWD_N, ab), what, key="embed_bwd: d_rows")
            R.assert_bits(d_bias, want_bias, what + ": d_bias")
        # in place, d_bias not wanted
        alias = dE_up.clone()
        ops.embed_bwd(alias, E=E, fm_sum=fm_sum, dE_up=alias, g_fm=g_fm, mask_b=mask_b, mask_e=mask_e)
        R.assert_bits(alias, d_rows_of(E, fm_sum, dE_up, g_fm, mask_b, mask_e), "d_rows aliasing dE_up")
    # no FM term
    d_rows, d_bias = _sentinel(B, F, D), _sentinel(B, F)
    ops.embed_bwd(d_rows, dE_up=dE_up, d_bias=d_bias)
    R.assert_bits(d_rows, dE_up, "g_fm NULL: d_rows = dE_up")
    R.assert_bits(d_bias, _sentinel(B, F), "g_fm NULL: d_bias untouched")


def d_rows_of(E, fm_sum, dE_up, g_fm, mask_b, mask_e):
    out = torch.empty_like(E)
    ops.embed_bwd(out, E=E, fm_sum=fm_sum, dE_up=dE_up, g_fm=g_fm, mask_b=mask_b, mask_e=mask_e)
    return out


@pytest.mark.parametrize("dist", ["distinct", "uniform", "hot"])
@pytest.mark.parametrize("form", ["rows-D", "rows-1", "g_row"])
def test_scatter_add_rows_against_float64(hip_lib, form, dist):
    """Float atomics in any order: n = multiplicity of the target row + 1 (its prior content is a term too).  Rows no
    occurrence touches, and the columns behind `width`, keep their bits (the kernel adds, it does not zero).
    distinct: every occurrence its own row (n = 2); hot: one row takes every occurrence of a field (n = B + 1)."""
    _cite_elementwise("embed.hip", "const int64_t total = B * F * width; dim3 grid(rm_grid_cap((total + kBlock - 1) / kBlock, 256 * 16));")
    F = 3
    width = 8 if form == "rows-D" else 1
    B = 70_001 if width == 8 else 400_003
    total = B * F * width
    assert total > ELEMENTWISE_THREADS and total % ELEMENTWISE_THREADS % KBLOCK != 0   # a second, ragged sweep
    g = _gen(len(form) + len(dist))
    V = B if dist == "distinct" else 1000
    field_off = torch.arange(F, device="cuda") * (V + 7)     # 7 rows per field that nothing touches
    if dist == "distinct":
        idx = torch.stack([torch.randperm(V, generator=g, device="cuda") for _ in range(F)], 1)
    else:
        idx = _randint(g, V, B, F)
        if dist == "hot":
            idx[:, 1] = 5
    idx = idx.contiguous()
    ld = width + 4
    prior = _randn(g, F * (V + 7), ld)
    d_table = prior.clone()
    # (the reference runs on the host: a float64 index_add of 400 003 terms into ONE address takes minutes on the device)
    if form == "g_row":
        g_row = _randn(g, B)
        ops.scatter_add_rows(d_table, idx, field_off, g_row=g_row, ld=ld)
        ref = R.scatter_add_ref(prior.cpu(), idx.cpu(), field_off.cpu(), 1, g_row=g_row.cpu())
    else:
        rows = _randn(g, B, F, width)
        ops.scatter_add_rows(d_table, idx, field_off, rows=rows, width=width, ld=ld)
        ref = R.scatter_add_ref(prior.cpu(), idx.cpu(), field_off.cpu(), width, rows=rows.cpu())
    want, ab, n, touched = (t.cuda() for t in ref)
    assert int(n.max()) == {"distinct": 2, "hot": B + 1}.get(dist, int(n.max())) and int((~touched).sum()) >= 7 * F
    R.assert_within(d_table, want, R.sum_bound(n, ab), f"scatter_add_rows {form} {dist}", key="scatter_add_rows")
    R.assert_bits(d_table[~touched], prior[~touched], "rows no occurrence touches")
    R.assert_bits(d_table[:, width:], prior[:, width:], "columns behind width")


def test_linear_fwd_against_float64(hip_lib):
    """n = F + Dn + 1.  One sweep is 256 * 8 blocks of 256 examples; F = 0 with Dn > 0, Dn = 0, w0 NULL."""
    _cite("embed.hip", "hipLaunchKernelGGL(linear_fwd_kernel, dim3(rm_grid_cap((B + kBlock - 1) / kBlock, 256 * 8)), dim3(kBlock)")
    sweep = 256 * 8 * KBLOCK
    assert sweep == 524_288
    g = _gen(11)
    for B, F, Dn, w0 in ((sweep + 37, 3, 2, True), (1, 26, 13, True), (257, 0, 13, True), (257, 5, 0, True),
                         (257, 5, 2, False), (2 * sweep + 1, 1, 0, False)):
        sizes = torch.tensor([3 + (7 * f) % 11 for f in range(F)], device="cuda", dtype=I64)
        lin_off = (torch.cumsum(sizes, 0) - sizes + 5).contiguous() if F else None
        idx = (torch.rand(B, F, generator=g, device="cuda") * sizes).long().clamp(max=sizes - 1).contiguous() if F else None
        if F:
            idx[0] = sizes - 1
        w = _randn(g, int(sizes.sum()) + 5) if F else None
        dense, w_dense = (_randn(g, B, Dn), _randn(g, Dn)) if Dn else (None, None)
        w0_t = _randn(g, 1) if w0 else None
        out = _sentinel(B)
        ops.linear_fwd(idx, lin_off, w, dense, w_dense, w0_t, out)
        if F:
            want, ab, n = R.linear_fwd_ref(idx, lin_off, w, dense, w_dense, w0_t)
        else:
            want, ab, n = R.linear_fwd_ref(None, None, None, dense, w_dense, w0_t)
        assert n == F + Dn + 1
        R.assert_within(out, want, R.sum_bound(n, ab), f"linear_fwd B={B} F={F} Dn={Dn} w0={w0}", key="linear_fwd")


def _colsum_path(Dn, aligned):
    """rm_linear_dense_bwd's choice of kernel (csrc/embed.hip): (path, Pp or None)."""
    if Dn >= 64 and Dn % 4 == 0 and aligned:
        return "wide", None
    Pp = 1
    while Pp < Dn + 1 and Pp < KBLOCK:
        Pp <<= 1
    return "narrow", Pp


DENSE_BWD_DN = [(0, True), (1, True), (13, True), (63, True), (64, True), (64, False), (255, True), (256, True),
                (400, True), (1023, True)]


@pytest.mark.parametrize("B", [1, 255, 257, 70_001])
def test_linear_dense_bwd_three_paths_against_float64(hip_lib, B):
    """n = B for every column and for d_w0.  Narrow kernel with Pp < 256 (Dn 0 .. 63, and Dn = 64 from a pointer one
    float off 16-byte alignment), with Dn + 1 > 256 (Dn = 1023: four column rounds) and at Pp = 256 exactly (255);
    wide float4 kernel (64 aligned, 256, 400) with its workspace-derived block cap.  Either output NULL; two runs
    bit-equal (fixed-order two-stage reduction)."""
    _linear_dense_bwd_case(B)


def _linear_dense_bwd_case(B):
    _cite("embed.hip", "if (Dn >= 64 && Dn % 4 == 0 && rm_aligned16(dense)) {")
    _cite("embed.hip", "const int64_t cap = 256 * 1024 / (Dn + 1);")
    _cite("embed.hip", "nblk = rm_grid_cap((B + 63) / 64, (int)(cap < 2048 ? cap : 2048));")
    _cite("embed.hip", "nblk = rm_grid_cap((B + 255) / 256, 256);")
    _cite("embed.hip", "while (Pp < Dn + 1 && Pp < kBlock) Pp <<= 1;")
    paths = [_colsum_path(Dn, al) for Dn, al in DENSE_BWD_DN]
    assert paths == [("narrow", 1), ("narrow", 2), ("narrow", 16), ("narrow", 64), ("wide", None), ("narrow", 128),
                     ("narrow", 256), ("wide", None), ("wide", None), ("narrow", 256)]
    assert cdiv(1023 + 1, 256) == 4                                  # column rounds of the narrow kernel at Dn = 1023
    if B == 70_001:
        assert min(cdiv(B, 64), 262_144 // 401, 2048) == 653        # Dn = 400: the workspace, not the batch, caps the blocks
        assert min(cdiv(B, 64), 262_144 // 65, 2048) == 1094        # Dn = 64: the batch does
        assert cdiv(B, 256) > 256                                    # narrow: 256 blocks of several row groups each
    g = _gen(B)
    ws = torch.empty(262_144, device="cuda")
    gg = _randn(g, B)
    outs = []
    for Dn, aligned in DENSE_BWD_DN:
        if Dn == 0:
            dense = None
        elif aligned:
            dense = _randn(g, B, Dn)
            assert dense.data_ptr() % 16 == 0
        else:
            buf = _randn(g, B * Dn + 4)
            dense = buf[1:1 + B * Dn].view(B, Dn)
            assert dense.data_ptr() % 16 == 4 and dense.is_contiguous()
        want, ab, want0, ab0 = R.linear_dense_bwd_ref(gg, dense)
        d_w = _sentinel(Dn) if Dn else None
        d_w0 = _sentinel(1)
        ops.linear_dense_bwd(gg, dense, d_w, d_w0, ws)
        what = f"linear_dense_bwd B={B} Dn={Dn} aligned={aligned}"
        path = _colsum_path(Dn, aligned)[0]
        if Dn:
            R.assert_within(d_w, want, R.sum_bound(B, ab), what, key=f"linear_dense_bwd {path}")
        R.assert_within(d_w0, want0, R.sum_bound(B, ab0), what + ": d_w0", key=f"linear_dense_bwd {path}")
        d_w2, d_w02 = (_sentinel(Dn) if Dn else None), _sentinel(1)
        ops.linear_dense_bwd(gg, dense, d_w2, None, ws)
        ops.linear_dense_bwd(gg, dense, None, d_w02, ws)
        R.assert_bits(d_w02, d_w0, what + ": d_w0 with d_w_dense NULL, second run")
        if Dn:
            R.assert_bits(d_w2, d_w, what + ": d_w_dense with d_w0 NULL, second run")
        outs.append((d_w, d_w0))
    return outs


# =================================================================================================================
# 3. loss and the small dense helpers
LOSS_CONFIGS = [  # (branch coefficients, task, label dtype)
    ((1.0,), "classification", I64),
    ((1.0, 2.0), "classification", F32),
    ((1.0, 1.0, -0.5), "regression", F32),
    ((1.0, 2.0, 1.0, 0.25), "regression", I64),
    ((0.5, 1.0, 1.0, -1.0), "classification", I64),
]


def _branches(z, coefs, g):
    """Branch logits whose weighted sum is about z (the reference sums the fp32 branches it is given)."""
    bs = [torch.randn(z.shape, generator=g) * 3 for _ in coefs[:-1]]
    last = (z - sum(c * b for c, b in zip(coefs, bs))) / coefs[-1]
    return [(b.float().cuda(), c) for b, c in zip(bs + [last], coefs)]


@pytest.mark.parametrize("B", [1, 262_145, 600_001])
@pytest.mark.parametrize("coefs,task,ydt", LOSS_CONFIGS, ids=lambda v: str(v).replace(" ", ""))
def test_logit_loss_against_float64(hip_lib, B, coefs, task, ydt):
    """logit: n = number of branches.  pred / dlogit / loss pass through expf and logf: rtol 1e-5, atol 1e-6 against
    float64 from the summed fp32 branches.  Body |z| <= 12; the clip region has its own test below.
    On top of that, tighter: B * dlogit and the loss against the float64 function of the fp32 probability the kernel
    wrote - Keras takes the cross-entropy from its fp32 sigmoid output, whose 1 - p is quantised to 2^-24 (0.5 % at
    |z| = 12), and dlogit / B at B = 600 001 would pass the absolute tolerance with any value."""
    _logit_loss_case(B, coefs, task, ydt)


def _logit_loss_case(B, coefs, task, ydt):
    _cite("loss.hip", "constexpr int kMaxBlocks = 1024;")
    _cite("loss.hip", "const int nblk = rm_grid_cap((B + kBlock - 1) / kBlock, kMaxBlocks);")
    sweep = 1024 * KBLOCK
    assert sweep == 262_144 and (B == 1 or (B > sweep and B % sweep % KBLOCK != 0))   # 262 145: 2 sweeps; 600 001: 3
    g = torch.Generator().manual_seed(B % 1000 + len(coefs))
    z = torch.rand(B, generator=g) * 24 - 12
    br = _branches(z, coefs, g)
    if task == "classification":
        y = (torch.rand(B, generator=g) < 0.4).to(ydt).cuda()
    else:
        y = (torch.randn(B, generator=g) * 3).round().to(ydt).cuda()
    kw = dict(y=y) if ydt == I64 else dict(y_f=y)
    ws = torch.empty(1024, device="cuda")
    out = dict(logit=_sentinel(B), pred=_sentinel(B), dlogit=_sentinel(B), loss=_sentinel(1))
    ops.logit_loss(br, task=task, workspace=ws, **kw, **out)
    z64, zab = R.logit_sum_ref(br)
    what = f"logit_loss B={B} {task} {len(coefs)} branches"
    R.assert_within(out["logit"], z64, R.sum_bound(len(coefs), zab), what + ": logit", key="logit_loss: logit")
    assert float(z64.abs().max()) <= 12.001
    p64, dz64, t64 = R.loss_point_ref(z64, y, task)
    R.close(out["pred"], p64, what=what + ": pred")
    R.close(out["dlogit"], dz64 / B, what=what + ": dlogit")
    R.close(out["loss"], t64.mean().reshape(1), what=what + ": loss")
    _, dzp, tp = R.loss_point_ref(out["logit"], y, task, pred=out["pred"])
    R.close(out["dlogit"].double() * B, dzp, what=what + ": B * dlogit from the fp32 probability")
    R.close(out["loss"], tp.mean().reshape(1), what=what + ": loss from the fp32 probability")
    # each optional output NULL in turn; the loss twice
    for skip in out:
        part = {k: _sentinel(*v.shape) for k, v in out.items() if k != skip}
        ops.logit_loss(br, task=task, workspace=ws if "loss" in part else None, **kw, **part)
        for k in part:
            R.assert_bits(part[k], out[k], f"{what}: {k} with {skip} = NULL (and run again)")
    return out


@pytest.mark.parametrize("ydt", [I64, F32], ids=["int64", "float"])
def test_logit_loss_clip_region(hip_lib, ydt):
    """|z| >= 20 with both labels: the probability lies outside [1e-7, 1 - 1e-7], the clip passes no gradient -
    dlogit exactly 0 - and pred is what fp32 gives: exactly 1 above, below 1e-7 and equal to the float64 sigmoid to
    tolerance below.  Nothing lies near the clip boundary (p = 1e-7 is |z| ~ 16.1): no example is left out."""
    B = 4099
    g = torch.Generator().manual_seed(5)
    z = (20 + torch.rand(B, generator=g) * 20) * torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0)
    z[:4] = torch.tensor([20.0, -20.0, 40.0, -40.0])
    y = (torch.rand(B, generator=g) < 0.5).to(ydt)
    y[:4] = torch.tensor([0, 1, 1, 0]).to(ydt)
    z, y = z.float().cuda(), y.cuda()
    out = dict(logit=_sentinel(B), pred=_sentinel(B), dlogit=_sentinel(B), loss=_sentinel(1))
    ops.logit_loss([(z, 1.0)], workspace=torch.empty(1024, device="cuda"), **(dict(y=y) if ydt == I64 else dict(y_f=y)),
                   **out)
    R.assert_bits(out["logit"], z, "logit of one branch with coefficient 1")
    R.assert_bits(out["dlogit"], torch.zeros(B, device="cuda"), "dlogit in the clip region")
    hi = z > 0
    R.assert_bits(out["pred"][hi], torch.ones(int(hi.sum()), device="cuda"), "pred above the clip")
    assert bool((out["pred"][~hi] < 1e-7).all()) and bool((out["pred"][~hi] > 0).all())
    p64, _, _ = R.loss_point_ref(z, y, "classification")
    R.close(out["pred"], p64, what="pred in the clip region")
    _, dz, t = R.loss_point_ref(z, y, "classification", pred=out["pred"])
    assert torch.equal(dz, torch.zeros_like(dz))
    R.close(out["loss"], t.mean().reshape(1), what="loss in the clip region")


@pytest.mark.parametrize("B", [1, 3, 5, 32_768 * 2 + 3])
def test_rowdot_against_float64(hip_lib, B):
    """n = P + 1.  P % 4 == 0 takes the float4 loop (P = 4, 60, 64, 68, 400: below, at and above one 64-column
    round of the 16 lanes), the others the scalar one; one sweep is 256 * 8 blocks of 4 waves of 4 rows."""
    _cite("loss.hip", "hipLaunchKernelGGL(rowdot_kernel, dim3(rm_grid_cap((B + 15) / 16, 256 * 8)), dim3(kBlock)")
    _cite("loss.hip", "for (int64_t b0 = wave * 4; b0 < B; b0 += nwaves * 4)")
    sweep = 256 * 8 * 4 * 4
    assert sweep == 32_768 and (B < 16 or (B > 2 * sweep and B % 4 == 3))
    g = _gen(B)
    for P in (1, 3, 4, 60, 64, 68, 400):
        X, w = _randn(g, B, P), _randn(g, P)
        for w0 in (_randn(g, 1), None):
            out = _sentinel(B)
            ops.rowdot(X, w, w0, out)
            want, ab = R.rowdot_ref(X, w, w0)
            R.assert_within(out, want, R.sum_bound(P + 1, ab), f"rowdot B={B} P={P} w0={'yes' if w0 is not None else 'NULL'}",
                            key="rowdot")


@pytest.mark.parametrize("act", ["identity", "relu", "leaky_relu"])
def test_bias_act_and_act_bwd_bit_for_bit(hip_lib, act):
    """One add and one select (leaky: one multiply) per element, no reassociation: bit for bit against the same
    expression in fp32 torch, at every element - exact zeros and negative zeros at the kink included."""
    _cite_elementwise("loss.hip", "const int64_t n4 = B * (N / 4); hipLaunchKernelGGL(bias_act_kernel, dim3(rm_grid_cap((n4 + kBlock - 1) / kBlock, 256 * 16))")
    _cite_elementwise("loss.hip", "const int64_t n4 = B * N / 4; hipLaunchKernelGGL(act_bwd_kernel, dim3(rm_grid_cap((n4 + kBlock - 1) / kBlock, 256 * 16))")
    g = _gen(len(act))
    for B, N in ((1, 4), (3, 400), (1_048_576 + 37, 4), (10_487, 400)):
        n4 = B * N // 4
        if B > 1000:
            assert n4 > ELEMENTWISE_THREADS and n4 % KBLOCK != 0        # a second, ragged sweep
        x, bias = _randn(g, B, N), _randn(g, N)
        bias[::3] = 0.0
        if N > 4:
            bias[1::7] = -0.0
        flat = x.view(-1)
        k = flat.numel()
        flat[0:k:5] = -bias.repeat(B)[0:k:5]        # x + bias == 0 exactly
        flat[1:k:11] = 0.0
        flat[2:k:13] = -0.0
        for bt in (bias, None):
            want = R.bias_act_ref32(x, bt, act)
            got = x.clone()
            ops.bias_act_(got, bt, act)
            R.assert_bits(got, want, f"bias_act {act} B={B} N={N} bias={'yes' if bt is not None else 'NULL'}")
            assert int((want == 0).sum()) >= k // 11
        a = R.bias_act_ref32(x, bias, act)
        a.view(-1)[3:k:17] = -0.0
        da = _randn(g, B, N)
        want = R.act_bwd_ref32(da, a, act)
        got = da.clone()
        ops.act_bwd_(got, a, act)
        R.assert_bits(got, want, f"act_bwd {act} B={B} N={N}")


# =================================================================================================================
# 4. row helpers and the router
ROW_CASES = [  # (width, n): n * G with G = width / 4
    (4, 1), (4, 7), (12, 7), (4, 8 * 1_048_576 + 5), (4, 3 * 1_048_576 + 1), (12, 2_796_203), (32, 1_048_577), (128, 262_145),
]


@pytest.mark.parametrize("width,n", ROW_CASES)
def test_gather_and_permute_rows_bit_for_bit(hip_lib, width, n):
    """Pure data movement.  rm_gather_rows takes 8 float4 per thread and iteration, stepping by 8 * stride and
    clamping the tail's index to total - 1: n * G = 8 388 608 + 5 starts a second unrolled sweep of which 5 float4 are
    real; a tenth of the rows are < 0 (zero rows out), the very last index - the one the clamp reads - among them.
    rm_permute_rows in both directions."""
    _cite("embed.hip", "constexpr int U = 8;")
    _cite("embed.hip", "for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t0 < total; t0 += U * stride)")
    _cite("embed.hip", "const int64_t i = (t < total ? t : total - 1) / G;")
    _cite_elementwise("embed.hip", "const int64_t total = n * G; dim3 grid(rm_grid_cap((total + kBlock - 1) / kBlock, 256 * 16)); hipLaunchKernelGGL(gather_rows_kernel")
    _cite_elementwise("embed.hip", "const int64_t total = n * G; dim3 grid(rm_grid_cap((total + kBlock - 1) / kBlock, 256 * 16)); hipLaunchKernelGGL(permute_rows_kernel")
    G = width // 4
    total = n * G
    if n > 1000:
        assert total > 3 * ELEMENTWISE_THREADS and total % ELEMENTWISE_THREADS != 0
    if (width, n) == (4, 8 * 1_048_576 + 5):
        assert total == 8 * ELEMENTWISE_THREADS + 5        # second unrolled sweep, 5 live float4, the rest clamped
    if n in (2_796_203, 1_048_577, 262_145):
        assert 8 * ELEMENTWISE_THREADS < total < 8 * ELEMENTWISE_THREADS + 64
    g = _gen(width + n % 1000)
    V, ld = 1000, width + 8
    table = _randn(g, V, ld)
    rows = _randint(g, V, n)
    rows[torch.rand(n, generator=g, device="cuda") < 0.1] = -1
    rows[n - 1] = -1
    rows[0] = V - 1
    out = _sentinel(n, width)
    ops.gather_rows(table, rows, out)
    R.assert_bits(out, R.gather_rows_ref(table, rows, width), f"gather_rows width={width} n={n}")
    rows[n - 1] = 0                                    # and with a real last row
    ops.gather_rows(table, rows, out)
    R.assert_bits(out, R.gather_rows_ref(table, rows, width), f"gather_rows width={width} n={n}, last row real")
    # permute: out (n rows) through a permutation and back
    slot = torch.randperm(n, generator=g, device="cuda")
    fwd = _sentinel(n, width)
    ops.permute_rows(out, slot, fwd)
    R.assert_bits(fwd, R.permute_rows_ref(out, slot, False, _sentinel(n, width)), "permute_rows")
    back = _sentinel(n, width)
    ops.permute_rows(out, slot, back, inverse=True)
    R.assert_bits(back, R.permute_rows_ref(out, slot, True, _sentinel(n, width)), "permute_rows inverse")
    del fwd
    again = _sentinel(n, width)
    ops.permute_rows(back, slot, again)
    R.assert_bits(again, out, "permute_rows undoes its inverse")


@pytest.mark.parametrize("B,F,D", [(1, 1, 4), (3, 7, 12), (257, 5, 32), (70_001, 5, 12), (2_049, 4, 128)])
def test_pack_grad_rows_bit_for_bit(hip_lib, B, F, D):
    """Data movement plus one fp32 multiply (g_lin * lin_field_mask).  Occurrences with pos = -1 are skipped: the
    slots they would have had keep their sentinel.  width in {D + 4, D + 12}: the columns behind D + 1 are zeros."""
    _cite_elementwise("route.hip", "const int64_t total = n * (width / 4); hipLaunchKernelGGL(pack_grad_rows_kernel, dim3(rm_grid_cap((total + kBlock - 1) / kBlock, 256 * 16))")
    _cite("route.hip", "if (pos[o] < 0) continue;")
    n = B * F
    if B == 70_001:
        assert n * (D + 4) // 4 > ELEMENTWISE_THREADS and (n * (D + 4) // 4) % KBLOCK != 0
    g = _gen(B + D)
    d_rows, gb, gl = _randn(g, B, F, D), _randn(g, B), _randn(g, B)
    lm = (torch.arange(F, device="cuda") % 3 != 1).float() * 1.5
    for width in (D + 4, D + 12):
        for share in (0.0, 0.2):
            valid = torch.rand(n, generator=g, device="cuda") >= share
            pos = torch.full((n,), -1, dtype=I64, device="cuda")
            pos[valid] = torch.randperm(n, generator=g, device="cuda")[: int(valid.sum())]
            for a_gb, a_gl, a_lm in ((gb, gl, lm), (gb, gl, None), (None, gl, lm), (gb, None, None), (None, None, None)):
                out = _sentinel(n, width)
                ops.pack_grad_rows(d_rows, a_gb, a_gl, pos, out, lin_field_mask=a_lm)
                want = R.pack_grad_rows_ref(d_rows, a_gb, a_gl, a_lm, pos, _sentinel(n, width))
                R.assert_bits(out, want, f"pack_grad_rows B={B} F={F} D={D} width={width} empty={share}")
            if share:
                assert int((out == -777.25).all(1).sum()) == n - int(valid.sum())


ROUTE_N = {255: (51, 5), 256: (64, 4), 257: (257, 1), 262_143: (87_381, 3), 262_144: (65_536, 4), 262_145: (52_429, 5),
           1_703_936 + 26: (65_537, 26)}


def _route_blocks(n):
    """shard_route_impl (csrc/route.hip): (blocks, occurrences per block)."""
    nblk = 1 if n == 0 else cdiv(n, 256) if n < 1024 * 256 else 1024
    return nblk, cdiv(cdiv(n, nblk), KBLOCK) * KBLOCK


def _route_inputs(n, g, negative, constant=False):
    B, F = ROUTE_N[n]
    sizes = torch.tensor([5 + (37 * f) % 1000 for f in range(F)], device="cuda", dtype=I64)
    field_off = (torch.cumsum(sizes, 0) - sizes).contiguous()
    idx = (torch.rand(B, F, generator=g, device="cuda") * sizes).long().clamp(max=sizes - 1)
    if constant:
        idx = torch.full((B, F), 3, dtype=I64, device="cuda")
        field_off = torch.zeros(F, dtype=I64, device="cuda")
    if negative >= 1.0:
        idx[:] = -1
    elif negative > 0:
        idx[torch.rand(B, F, generator=g, device="cuda") < negative] = -1
    return idx.contiguous(), field_off


@pytest.mark.parametrize("world", [1, 2, 3, 8, 16])
def test_shard_route_against_the_torch_router(hip_lib, world):
    """pos / send_ids / counts bit-equal to recman_amd.dist.route_torch.  From n = 262 144 the router runs 1 024 blocks;
    past it every block walks several 256-occurrence chunks and route_place_kernel carries a running offset per bucket
    from chunk to chunk (n = 262 145: 2 chunks; 1 703 962: 7)."""
    _cite("route.hip", "const int nblk = (int)(n == 0 ? 1 : n < 1024 * 256 ? (n + 255) / 256 : 1024);")
    _cite("route.hip", "const int64_t per_block = ((n + nblk - 1) / nblk + kBlock - 1) / kBlock * kBlock;")
    _cite("route.hip", "for (int64_t ob = o0; ob < o1; ob += kBlock) {")
    assert [_route_blocks(n) for n in ROUTE_N] == [(1, 256), (1, 256), (2, 256), (1024, 256), (1024, 256), (1024, 512),
                                                   (1024, 1792)]
    ws = torch.empty(int(_lib.lib().rm_shard_route_workspace(world)), dtype=torch.int32, device="cuda")
    g = _gen(world)
    for n, (B, F) in ROUTE_N.items():
        assert B * F == n
        cases = [(0.0, False)]
        if n in (257, 262_145, 1_703_936 + 26):
            cases += [(0.1, False), (1.0, False), (0.0, True)]
        for negative, constant in cases:
            idx, field_off = _route_inputs(n, g, negative, constant)
            _shard_route_case(idx, field_off, world, ws, constant, f"n={n} negative={negative} constant={constant}")


def _shard_route_case(idx, field_off, world, ws, constant, tag):
    n = idx.numel()
    pos, send, counts = (torch.full((n,), -5, dtype=I64, device="cuda"), torch.full((n,), -5, dtype=I64, device="cuda"),
                         torch.full((world,), -5, dtype=I64, device="cuda"))
    ops.shard_route(idx, field_off, world, pos, send, counts, ws)
    pos_t, counts_t, send_t = route_torch(idx, field_off, world)
    what = f"shard_route world={world} {tag}"
    assert torch.equal(counts, counts_t), what + ": counts"
    assert torch.equal(pos, pos_t), what + ": pos"
    nv = send_t.numel()
    assert nv == int((idx >= 0).sum()) and torch.equal(send[:nv], send_t), what + ": send_ids"
    if constant:
        assert int((counts > 0).sum()) == 1 and int(counts.sum()) == n   # every id owned by one rank
    return pos, send[:nv], counts


def _shard_route_padded_run(idx, field_off, world, c, over, ws):
    n = idx.numel()
    pos, send, counts = (torch.full((n,), -5, dtype=I64, device="cuda"),
                         torch.full((world * c,), -5, dtype=I64, device="cuda"),
                         torch.full((world,), -5, dtype=I64, device="cuda"))
    ops.shard_route_padded(idx, field_off, world, c, pos, send, counts, over, ws)
    return pos, send, counts


@pytest.mark.parametrize("world", [1, 2, 3, 8, 16])
def test_shard_route_padded_capacity_and_sticky_overflow(hip_lib, world):
    """Fixed-capacity buckets against route_torch(cap): a capacity that fits exactly (flag stays 0); one slot too few
    (flag 1, every pos inside world * cap, pos bit-equal to the reference's clamped ones, every bucket that fits still
    exact in send_ids); the flag stays set across a second, fitting call until the caller clears it."""
    ws = torch.empty(int(_lib.lib().rm_shard_route_workspace(world)), dtype=torch.int32, device="cuda")
    g = _gen(50 + world)
    for n in (257, 262_145, 1_703_936 + 26):
        for negative, constant in ((0.0, False), (0.1, False), (0.0, True)):
            idx, field_off = _route_inputs(n, g, negative, constant)
            _, counts_t, _ = route_torch(idx, field_off, world)
            cap = int(counts_t.max())
            over = torch.zeros(1, dtype=torch.int32, device="cuda")

            def run(c):
                return _shard_route_padded_run(idx, field_off, world, c, over, ws)

            what = f"shard_route_padded world={world} n={n} negative={negative} constant={constant}"
            pos, send, counts = run(cap)
            pos_t, counts_t, send_t, over_t = route_torch(idx, field_off, world, cap)
            assert int(over) == 0 and int(over_t) == 0, what
            assert torch.equal(pos, pos_t) and torch.equal(send, send_t) and torch.equal(counts, counts_t), what
            if cap < 2:
                continue
            pos, send, counts = run(cap - 1)
            pos_t, counts_t, send_t, over_t = route_torch(idx, field_off, world, cap - 1)
            assert int(over) == 1 and int(over_t) == 1, what + ": one slot too few"
            assert int(pos.max()) < world * (cap - 1) and torch.equal(pos, pos_t) and torch.equal(counts, counts_t), what
            fits = (counts_t <= cap - 1).repeat_interleave(cap - 1)     # slots of the buckets that fit
            assert torch.equal(send[fits], send_t[fits]), what + ": buckets that fit"
            last = torch.arange(1, world + 1, device="cuda") * (cap - 1) - 1
            rest = ~fits
            rest[last] = False                                          # (the clamped slot has several writers)
            assert torch.equal(send[rest], send_t[rest]), what + ": overflowing buckets below their last slot"
            pos, send, counts = run(cap)                                # fits again: the flag is sticky
            assert int(over) == 1 and torch.equal(pos, route_torch(idx, field_off, world, cap)[0]), what + ": sticky"
            over.zero_()
            run(cap)
            assert int(over) == 0, what + ": cleared"


# =================================================================================================================
# 5. pooling
def _pool_case(B, D, LD, row0, seed, with_vals):
    g = _gen(seed)
    V = 50
    cnt = _randint(g, 6, B)
    lead = torch.tensor([0, 1, 4, 33], device="cuda")[: min(4, B)]
    cnt[: lead.numel()] = lead
    if B == 1:
        cnt[0] = 33
    offsets = torch.zeros(B + 1, dtype=I64, device="cuda")
    offsets[1:] = torch.cumsum(cnt, 0)
    nnz = int(offsets[-1])
    ids = _randint(g, V, nnz)
    ids[::3] = 0                                  # id 0 among the tags: the linear column drops it, the embedding keeps it
    rows = _randn(g, row0 + V, LD)
    vals = _randn(g, nnz) if with_vals else None
    return g, V, cnt, offsets, ids, rows, vals


def _check_pooled(got, want, ab, cnt, D, LD, sqrtn, what, key):
    """sqrtn form: columns 0 .. D carry the rsqrtf factor - the project's tolerance; the linear column (and every
    column of the vals form) is a plain sum: n = the example's tag count.  Columns D + 2 .. LD - 1 are zeros."""
    if sqrtn:
        R.close(got[:, :D + 1], want[:, :D + 1], what=what + ": sqrtn columns")
        R.assert_within(got[:, D + 1], want[:, D + 1], R.sum_bound(cnt, ab[:, D + 1]), what + ": linear column", key=key)
    else:
        R.assert_within(got[:, :D + 2], want[:, :D + 2], R.sum_bound(cnt[:, None], ab[:, :D + 2]), what, key=key)
    R.assert_bits(got[:, D + 2:], torch.zeros(got.shape[0], LD - D - 2, device="cuda"), what + ": columns behind D + 1")
    empty = cnt == 0
    R.assert_bits(got[empty], torch.zeros(int(empty.sum()), LD, device="cuda"), what + ": empty examples")


POOL_SHAPES = [(8, 12), (8, 16), (16, 20), (16, 32), (64, 68), (64, 128)]  # LD = D + 2 rounded up to 4, 2 D, 20 with 16


@pytest.mark.parametrize("with_vals", [False, True], ids=["sqrtn", "vals"])
@pytest.mark.parametrize("B", [1, 100_003])
@pytest.mark.parametrize("D,LD", POOL_SHAPES)
def test_pool_rows_forward_and_backward_against_float64(hip_lib, D, LD, B, with_vals):
    """rm_pool_rows / rm_pool_rows_bwd (CSR) and rm_pool_rows_padded / rm_pack_pooled_grad_rows (padded columns)
    against float64.  Tag counts 0, 1, 4, 33; row0 > 0; backward: float atomics, n = multiplicity of the tag's row + 1
    (+ RSQRT_TERMS in the sqrtn form, whose every term carries the rsqrtf factor).  At B = 100 003 a row takes about
    5 000 terms, and a tolerance relative to the result's size is not made for such sums: rtol 1e-5 / atol 1e-6 was
    tried first and the kernel measured 4.3e-3 on a result of 377, 1.14 of it - fp32 summation, not an error.  Rows no
    tag touches keep their bits."""
    assert LD in ((D + 2 + 3) // 4 * 4, 2 * D, 20)
    row0 = 3
    g, V, cnt, offsets, ids, rows, vals = _pool_case(B, D, LD, row0, D + LD + B % 100, with_vals)
    form = "vals" if with_vals else "sqrtn"
    what = f"pool_rows D={D} LD={LD} B={B} {form}"
    out = _sentinel(B, LD)
    ops.pool_rows(rows, row0, D, offsets, ids, out, vals=vals)
    want, ab, cnt_r = R.pool_rows_ref(rows, row0, D, offsets, ids, vals)
    assert torch.equal(cnt_r, cnt) and (B == 1 or cnt[:4].tolist() == [0, 1, 4, 33])
    _check_pooled(out, want, ab, cnt, D, LD, not with_vals, what, f"pool_rows {form}")
    # backward into non-zero buffers
    Rn = row0 + V + 2
    d_rows_wide = _randn(g, B, D + 4)
    gb, gl = _randn(g, B), _randn(g, B)
    prior = _randn(g, Rn, D), _randn(g, Rn), _randn(g, Rn)
    bufs = [p.clone() for p in prior]
    ops.pool_rows_bwd(d_rows_wide[:, :D], gb, gl, D, offsets, ids, row0, *bufs, vals=vals)
    refs = R.pool_rows_bwd_ref(d_rows_wide, gb, gl, D, offsets, ids, vals, row0, *prior)
    for name, got, pr, (res, rab, n) in zip(("d_table", "d_bias", "d_lin"), bufs, prior, refs):
        # sqrtn: every term of d_table / d_bias carries rsqrtf(count), 1 ulp: n + RSQRT_TERMS (d_lin has no factor)
        extra = 0 if with_vals or name == "d_lin" else R.RSQRT_TERMS
        R.assert_within(got, res, R.sum_bound(n + extra, rab), f"{what} bwd: {name}", key=f"pool_rows_bwd {form}")
        untouched = (n.reshape(Rn, -1)[:, 0] == 1)
        assert int(untouched.sum()) >= row0 + 2
        R.assert_bits(got[untouched], pr[untouched], f"{what} bwd: {name} rows no tag touches")
    only_t = prior[0].clone()
    ops.pool_rows_bwd(d_rows_wide[:, :D], None, gl, D, offsets, ids, row0, only_t, None, None, vals=vals)
    R.assert_within(only_t, refs[0][0], R.sum_bound(refs[0][2] + (0 if with_vals else R.RSQRT_TERMS), refs[0][1]),
                    what + " bwd: d_table alone")
    # padded form: tags as columns (holes in odd examples), rows addressed through positions
    T = 34
    nnz = ids.numel()
    seg = torch.repeat_interleave(torch.arange(B, device="cuda"), cnt)
    col = torch.arange(nnz, device="cuda") - offsets[seg] + (seg % 2) * (cnt[seg] < T).long()
    pid = torch.full((B, T), -1, dtype=I64, device="cuda")
    pid[seg, col] = ids
    slots = nnz + 3
    perm = torch.randperm(slots, generator=g, device="cuda")[:nnz]
    ppos = torch.full((B, T), -1, dtype=I64, device="cuda")
    ppos[seg, col] = perm
    recv = _randn(g, slots, LD)
    recv[perm] = rows[row0 + ids]
    pvals = None
    if with_vals:
        pvals = torch.zeros(B, T, device="cuda")
        pvals[seg, col] = vals
    outp = _sentinel(B, LD)
    ops.pool_rows_padded(recv, D, ppos, pid, outp, vals=pvals)
    wantp, abp, cntp = R.pool_rows_padded_ref(recv, D, ppos, pid, pvals)
    assert torch.equal(cntp, cnt)
    _check_pooled(outp, wantp, abp, cnt, D, LD, not with_vals, what + " padded", f"pool_rows_padded {form}")
    R.assert_bits(outp, out, what + ": padded = CSR (same sums in the same order)")
    for width in (D + 4, LD):
        sent = _sentinel(slots, width)
        packed = sent.clone()
        ops.pack_pooled_grad_rows(d_rows_wide[:, :D], gb, gl, D, ppos, pid, packed, vals=pvals)
        wantk = R.pack_pooled_grad_rows_ref(d_rows_wide, gb, gl, D, ppos, pid, pvals, sent)
        if with_vals:   # one fp32 product per element: n = 1
            R.assert_within(packed, wantk, R.sum_bound(1, wantk.abs()), what + " pack_pooled_grad_rows",
                            key="pack_pooled_grad_rows vals")
        else:
            R.close(packed, wantk, what=what + " pack_pooled_grad_rows")
        used = torch.zeros(slots, dtype=torch.bool, device="cuda")
        used[perm] = True
        R.assert_bits(packed[~used], sent[~used], what + ": slots no tag owns")
        R.assert_bits(packed[used][:, D + 2:], torch.zeros(nnz, width - D - 2, device="cuda"), what + ": pad columns")


# =================================================================================================================
# 6. element offsets beyond 2^31
def test_row_offsets_beyond_2_to_31(hip_lib):
    """A fused-row table with LD = 256 and 8 392 704 rows (8.6 GB): the top rows start at element offsets above 2^31.
    Ids in the top rows must return the top rows' values through rm_embed_fwd (fused, D = 128), rm_gather_rows and
    rm_scatter_add_rows; the rows at the 32-bit aliases of their offsets (row - 2^31 / LD) hold other values and must
    neither be read nor written.  Only the rows the batch touches and their aliases are initialised."""
    LD, D, top = 256, 128, 1024
    alias = 2 ** 31 // LD
    Rn = alias + 4096
    need = Rn * LD * 4 + (2 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of free device memory, the device reports {free / 2 ** 30:.1f}")
    assert (Rn - top) * LD > 2 ** 31 and need < 11 * 2 ** 30
    g = _gen(64)
    table = torch.empty(Rn, LD, device="cuda")
    try:
        table[Rn - top:] = _randn(g, top, LD)
        table[Rn - top - alias: Rn - alias] = _randn(g, top, LD) + 100.0      # the aliases: different values
        B = 513
        idx = torch.stack([Rn - top + _randint(g, top, B), _randint(g, top, B)], 1).contiguous()
        idx[0, 0], idx[0, 1] = Rn - 1, top - 1
        field_off = torch.tensor([0, Rn - top], device="cuda")
        out = dict(E=_sentinel(B, 2, D), fm_sum=_sentinel(B, D), fm_logit=_sentinel(B), lin_logit=_sentinel(B))
        ops.embed_fwd(idx, table, field_off, table_ld=LD, D=D, bias_col=D, lin_col=D + 1, **out)
        assert _runs_fused(D, LD, True, True, True, True)
        flat = table.reshape(-1)
        ref = R.embed_fwd_ref(idx, table, field_off, D, bias=flat[D:], bias_ld=LD, lin=flat[D + 1:], lin_ld=LD,
                              lin_off=field_off)
        assert bool((ref["E"].abs() < 50).all())                                 # (none of the + 100 alias rows)
        R.assert_bits(out["E"], ref["E"], "E from rows beyond 2^31")
        R.assert_within(out["fm_sum"], ref["fm_sum"], R.sum_bound(2, ref["fm_sum_abs"]), "fm_sum beyond 2^31")
        R.assert_within(out["fm_logit"], ref["fm_logit"], ref["fm_logit_bound"], "fm_logit beyond 2^31")
        R.assert_within(out["lin_logit"], ref["lin_logit"], R.sum_bound(3, ref["lin_abs"]), "lin_logit beyond 2^31")
        # the unfused kernel on the same rows (no bias, no linear weight: not the fused dispatch)
        E2 = _sentinel(B, 2, D)
        ops.embed_fwd(idx, table, field_off, table_ld=LD, D=D, E=E2)
        assert not _runs_fused(D, LD, True, True, False, False)
        R.assert_bits(E2, ref["E"], "E from rows beyond 2^31, unfused kernel")
        rows = (idx + field_off).reshape(-1).contiguous()
        got = _sentinel(rows.numel(), D)
        ops.gather_rows(table, rows, got)
        R.assert_bits(got, table[rows][:, :D], "gather_rows beyond 2^31")
        # scatter into the top rows of the same buffer (width D, ld LD)
        prior_top, prior_alias = table[Rn - top:].clone(), table[Rn - top - alias: Rn - alias].clone()
        add = _randn(g, B, 2, D)
        ops.scatter_add_rows(table, idx, field_off, rows=add, width=D, ld=LD)
        want = prior_top.double()
        want[:, :D] = want[:, :D].index_add(0, rows - (Rn - top), add.double().reshape(-1, D))
        ab = prior_top.double().abs()
        ab[:, :D] = ab[:, :D].index_add(0, rows - (Rn - top), add.double().abs().reshape(-1, D))
        n = torch.bincount(rows - (Rn - top), minlength=top)[:, None] + 1
        R.assert_within(table[Rn - top:], want, R.sum_bound(n, ab), "scatter_add_rows beyond 2^31")
        R.assert_bits(table[Rn - top - alias: Rn - alias], prior_alias, "the 32-bit aliases of the scattered rows")
    finally:
        del table
        torch.cuda.empty_cache()


# =================================================================================================================
# 7. dense optimizer
@pytest.mark.parametrize("kind", ["adam", "adagrad", "sgd"])
@pytest.mark.parametrize("n", [1, 3, 262_144 + 1, 1_000_003])
def test_dense_optimizer_step_against_float64(hip_lib, kind, n):
    """Keras Adam / Adagrad / SGD on a flat buffer against the float64 restatement, steps 1, 2 and 1000 on carried
    state, then a `reset` step (passed step = 3) that must ignore the stored moments AND the step number: a new
    optimizer's first step, as include/recman_hip.h states.  One step has no long sum: the tolerance of
    test_fused_dense_optimizer_equals_the_per_tensor_one, 2e-6 * max(1, max|.|), for the parameters and the moments
    written back.  One sweep is 256 * 4 blocks of 256 elements."""
    _cite("optim.hip", "hipLaunchKernelGGL(dense_opt_kernel, dim3(rm_grid_cap((n + kBlock - 1) / kBlock, 256 * 4)), dim3(kBlock)")
    sweep = 256 * 4 * KBLOCK
    assert sweep == 262_144 and (n < 4 or n == sweep + 1 or (n > 3 * sweep and n % KBLOCK != 0))
    g = _gen(n % 997 + len(kind))
    p = _randn(g, n)
    m = torch.zeros(n, device="cuda") if kind == "adam" else None
    v = None if kind == "sgd" else torch.full((n,), 0.1 if kind == "adagrad" else 0.0, device="cuda")
    p64 = p.double()
    m64 = None if m is None else m.double()
    v64 = None if v is None else v.double()

    def tol(got, want, what):
        err = float((got.double() - want).abs().max())
        assert err <= 2e-6 * max(1.0, float(want.abs().max())), f"{what}: max err {err:.3e}"

    for step, reset in ((1, False), (2, False), (1000, False), (3, True)):
        grad = _randn(g, n) * 0.5
        if reset:       # junk in the stored moments: a reset step must not read them
            if m is not None:
                m.fill_(123.0)
            if v is not None:
                v.fill_(456.0)
        ops.dense_optimizer_step(p, grad, m, v, step, kind, 0.01, reset=reset)
        p64, m64, v64 = R.dense_opt_ref(p64, grad, m64, v64, step, kind, 0.01, reset=reset)
        what = f"dense_optimizer_step {kind} n={n} step={step} reset={reset}"
        tol(p, p64, what + ": p")
        if m is not None:
            tol(m, m64, what + ": m")
        if v is not None:
            tol(v, v64, what + ": v")


# =================================================================================================================
def test_zz_error_to_bound_ratios(hip_lib):
    """Prints the largest |error| / bound ratio each summing kernel reached in this run (run with -s).  Near 1: the
    bound has no slack; below 1e-3 everywhere: a tighter check would be possible."""
    for k in sorted(R.RATIOS):
        print(f"[err/bound] {k:40s} {R.RATIOS[k]:.4f}")
    assert all(r <= 1.0 for r in R.RATIOS.values())
