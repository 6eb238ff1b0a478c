"""The epilogue of the direct implicit-GEMM kernel (fd_conv_epilogue.inc, fd_conv_res_prefetch.inc): the straight-line store loop per (residual, activation)
variant and the 32-bit buffer addressing of its stores and residual loads -- at the smallest shapes at which either can go wrong (a ragged last M tile with two
levels inside one tile, a cut 32-channel block, every tile the kernel is built for, every epilogue and kernel variant, channel views).  Outputs go into NaN-filled
buffers with guard rows: nothing outside the view may be written, every pixel inside must be.  Every case is checked against an fp64 F.conv2d reference at the
bound of test_conv_geometry_gpu (atol 1e-4 + rtol 1e-5), and bit for bit between two runs and between the 32-bit arm and the pointer arm (a view whose row
stride is too large for 32-bit offsets)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd._lib import ACT_EXP, ACT_NONE, ACT_RELU, ACT_SILU, Segs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL, RTOL = 1e-4, 1e-5         # test_conv_geometry_gpu's bar of the fp32 direct kernel
GUARD = 8                       # rows of NaN in front of and behind every output view: a row past M that was stored would land there
B = 2
PYRAMID = [(9, 7), (5, 6)]      # 186 rows: a ragged last M tile on every tile height, rows 126 .. 127 of the first 128-row tile belong to the second level
BIG_CS = 1 << 20                # a row stride at which 256 rows past the view no longer fit 32-bit byte offsets: the launch takes the pointer arm
DIRECT_TILES = [t for t in sorted(_lib.TILES) if t not in (_lib.PATCH_TILE, _lib.WAVE_TILE)]      # one-, two- and four-sub-tile waves, single and double buffer
PRM = [1.2, 0.9]

# name -> (levels, k, stride, pad)
GEOMS = {"pw_pyramid": (PYRAMID, 1, 1, 0), "s2_3x3": ([(9, 7)], 3, 2, 1)}
# name -> (act, act_c0, per-level parameter, residual, ReLU-mask residual)
EPILOGUES = {
    "none": (ACT_NONE, 0, False, False, False),
    "relu_all": (ACT_RELU, 0, False, False, False),
    "silu_all": (ACT_SILU, 0, False, False, False),
    "relu_from_c20": (ACT_RELU, 20, False, False, False),      # act_c0 inside the first 32-channel block: the general arm there, the fast arm behind it
    "residual_relu": (ACT_RELU, 0, False, True, False),
    "relu_mask": (ACT_NONE, 0, False, True, True),             # the data-gradient epilogue
    "scale_exp": (ACT_EXP, 4, True, False, False),             # a different seg_param per level
    "residual_none": (ACT_NONE, 0, False, True, False),        # ... and the rest of the fast loop's nine (residual, activation) copies
    "residual_silu": (ACT_SILU, 0, False, True, False),
    "relu_mask_relu": (ACT_RELU, 0, False, True, True),
    "relu_mask_silu": (ACT_SILU, 0, False, True, True),
}


def rows_of(ts):
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in ts])


def out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


_big = {}


def guarded(rows, C, cs=None):
    """A NaN-filled [rows + 2 * GUARD, cs] buffer and the [rows, C] view at channel 4 of its middle rows.  The BIG_CS buffer (0.8 GB) is allocated once."""
    cs = cs or C + 8
    if cs == BIG_CS:
        buf = _big.get(rows)
        if buf is None:
            _big.clear()
            torch.cuda.empty_cache()
            buf = _big[rows] = torch.empty(rows + 2 * GUARD, cs, device=DEV)
        buf.fill_(float("nan"))
    else:
        buf = torch.full((rows + 2 * GUARD, cs), float("nan"), device=DEV)
    return buf, ops.Rows(buf[GUARD:GUARD + rows], 4, C)


def launch(make_run, rows, C, cs=None, written=None):
    """Run make_run(y) into a fresh guarded view; returns the [rows, C] result after checking that nothing outside was written and everything inside was
    (`written`: the rows a scatter launch writes)."""
    buf, y = guarded(rows, C, cs)
    make_run(y)()
    torch.cuda.synchronize()
    got = y.tensor()
    nan = torch.isnan(buf)
    inside = int(nan[GUARD:GUARD + rows, 4:4 + C].sum())
    assert int(nan.sum()) - inside == buf.numel() - rows * C, "wrote outside its channel view / rows"
    if written is None:
        assert inside == 0, "an output pixel was never written"
    else:
        assert bool((~nan[GUARD:GUARD + rows, 4:4 + C][written]).all()), "an output pixel was never written"
        assert inside == (rows - int(written.sum())) * C, "a scatter launch wrote a row that is not its own"
    return got.clone()


def close(got, ref, what):
    g = got.double().cpu()
    err = (g - ref).abs()
    print(f"{what}: max|err| {float(err.max()):.3e} rel {float(err.max()) / (float(ref.abs().max()) + 1e-12):.3e}")
    np.testing.assert_allclose(g.numpy(), ref.numpy(), atol=ATOL, rtol=RTOL, err_msg=what)


class Case:
    """Inputs and the fp64 reference of one (geometry, Cout, epilogue): computed once, shared by the tiles, never modified."""

    def __init__(self, geom, Cout, epi, Cin=32):
        hw, k, stride, pad = GEOMS[geom]
        act, act_c0, per_level, use_res, mask = EPILOGUES[epi]
        gen = torch.Generator().manual_seed(100 * Cout + 10 * len(geom) + len(epi) + Cin)
        self.segs, self.Cout = Segs.make(B, hw), Cout
        xs = [torch.randn(B, Cin, h, w, generator=gen) for h, w in hw]
        wt = torch.randn(Cout, Cin, k, k, generator=gen) / (Cin * k * k) ** 0.5
        sc, sf = torch.rand(Cout, generator=gen) + 0.5, torch.randn(Cout, generator=gen) * 0.1
        rs = [torch.randn(B, Cout, *out_hw(h, w, k, stride, pad), generator=gen) for h, w in hw]
        ref = []
        for lv, (x, r) in enumerate(zip(xs, rs)):
            y = F.conv2d(x.double(), wt.double(), None, stride, pad) * sc.double()[None, :, None, None] + sf.double()[None, :, None, None]
            if use_res:
                y = torch.where(r.double() > 0, y, torch.zeros_like(y)) if mask else y + r.double()
            a = {ACT_NONE: y, ACT_RELU: F.relu(y), ACT_SILU: F.silu(y), ACT_EXP: torch.exp(y * PRM[lv])}[act]
            ref.append(torch.cat([y[:, :act_c0], a[:, act_c0:]], 1))
        self.ref = rows_of(ref)
        self.rows = self.ref.shape[0]
        xb = torch.full((self.segs.rows, Cin + 8), float("nan"), device=DEV)
        xb[:, 4:4 + Cin] = rows_of(xs).to(DEV)
        rb = torch.full((self.rows, Cout + 4), float("nan"), device=DEV)
        rb[:, 4:] = rows_of(rs).to(DEV)                        # the residual is a channel view at offset 4
        self.x, self.wp = ops.Rows(xb, 4, Cin), ops.pack_conv_weight(wt.to(DEV))
        self.kw = dict(Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, scale=sc.to(DEV), shift=sf.to(DEV), res=ops.Rows(rb, 4, Cout) if use_res else None,
                       res_mask=mask, act=act, act_c0=act_c0, seg_param=PRM[:len(hw)] if per_level else None)

    def run(self, y, **more):
        return ops.conv_call(self.x, self.segs, self.wp, y, **{**self.kw, **more})

    def launch(self, cs=None, **more):
        return launch(lambda y: self.run(y, **more), self.rows, self.Cout, cs)


_cases = {}


def case_of(*key, **kw):
    k = key + tuple(sorted(kw.items()))
    if k not in _cases:
        _cases[k] = Case(*key, **kw)
    return _cases[k]


@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("Cout", [64, 40, 96])       # full 32-channel blocks; a cut block (the column-edge arm); three blocks (128 x 96, a dead block elsewhere)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_every_tile_of_every_epilogue(geom, Cout, epi):
    c = case_of(geom, Cout, epi)
    for tile in DIRECT_TILES:
        first = c.launch(tile=tile)
        close(first, c.ref, f"{geom} Cout {Cout} {epi} tile {tile}")
        assert torch.equal(c.launch(tile=tile), first), f"tile {tile}: two runs differ"
        assert torch.equal(c.launch(cs=BIG_CS, tile=tile), first), f"tile {tile}: the 32-bit arm and the pointer arm differ"


def test_view_too_large_for_32_bit_offsets():
    """An output view of more than 3 GiB (few rows, a huge row stride) takes the pointer arm: the same bits as the compact view, nothing written outside."""
    c = case_of("pw_pyramid", 64, "residual_relu")
    first = c.launch(tile=1)
    _big.clear()
    torch.cuda.empty_cache()
    cs = 4_400_000                                   # 186 rows: 3.27 GB, under the entry point's 2^31 elements
    assert (c.rows - 1) * cs * 4 >= 0xC0000000 and c.rows * cs < 2 ** 31
    buf = torch.full((c.rows, cs), float("nan"), device=DEV)
    y = ops.Rows(buf, cs - c.Cout - 4, c.Cout)
    c.run(y, tile=1)()
    torch.cuda.synchronize()
    assert torch.equal(y.tensor(), first)
    assert int(torch.isnan(buf).sum()) == buf.numel() - first.numel(), "wrote outside its channel view"
    del buf, y
    torch.cuda.empty_cache()


@pytest.mark.parametrize("geom,Cin", [("pw_pyramid", 64), ("s2_3x3", 32)])
def test_split_k_slabs(geom, Cin):
    """Split-K 2: raw partial sums through the same epilogue into the two slabs of a NaN-filled workspace (the slice offset folded into the descriptor's base, the
    slab's extent its bound), the combine launch applies the epilogue.  Nothing behind the two slabs; the fp64 bound; two runs bit for bit."""
    c = case_of(geom, 40, "residual_relu", Cin=Cin)
    for tile in (1, 4, 8, 10):
        ws = torch.full((2 * c.rows * 40 + 64,), float("nan"), device=DEV)
        got = c.launch(tile=tile, ksplit=2, workspace=ws)
        close(got, c.ref, f"{geom} split-K tile {tile}")
        assert not bool(torch.isnan(ws[:2 * c.rows * 40]).any()), "a slab element was never written"
        assert bool(torch.isnan(ws[2 * c.rows * 40:]).all()), "wrote behind the two slabs"
        assert torch.equal(c.launch(tile=tile, ksplit=2, workspace=ws), got), "two split-K runs differ"


def test_scatter_launch():
    """sc_on: output pixel (i, j) of a 9 x 7 map goes to (2 i + 1, 2 j) of an 18 x 14 map and reads the residual THERE -- the pointer arm of the prefetch and of
    the stores, behind the row decode.  The written rows hold, bit for bit, what the plain launch stores with the same residual values in its own row order; no
    other row is touched, and the residual rows that are no target (NaN) are never read into a result."""
    c = case_of("s2_3x3", 64, "relu_all")          # (its inputs and filter, run here as a stride-1 'same' conv: 126 output rows)
    H, W, SH, SW = 9, 7, 18, 14
    kw = dict(stride=1, pad=1)
    n, i, j = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
    dst = ((n * SH + 2 * i + 1) * SW + 2 * j).reshape(-1).to(DEV)
    written = torch.zeros(B * SH * SW, dtype=torch.bool, device=DEV)
    written[dst] = True
    r = torch.randn(B * H * W, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    rp = torch.full((B * H * W, 68), float("nan"), device=DEV)
    rp[:, 4:] = r
    rs = torch.full((B * SH * SW, 68), float("nan"), device=DEV)
    rs[dst, 4:] = r
    for tile in (1, 4, 9):
        plain = launch(lambda y: c.run(y, tile=tile, res=ops.Rows(rp, 4, 64), **kw), B * H * W, 64)
        got = launch(lambda y: c.run(y, tile=tile, res=ops.Rows(rs, 4, 64), scatter=(2, 2, 1, 0, SH, SW), **kw), B * SH * SW, 64, written=written)
        assert torch.equal(got[dst], plain), f"tile {tile}: the scattered rows differ from the plain launch"
    nores = launch(lambda y: c.run(y, tile=4, **kw), B * H * W, 64)
    assert not torch.equal(nores, plain), "the residual did not reach the result"


@pytest.mark.parametrize("tile", [4, 7, 8, 9])
def test_k_concatenated_second_source(tile):
    """x2 (the DUAL instantiations): y = relu(a . Wa^T + b[::2, ::2] . Wb^T + shift) on a 9 x 7 map, 126 rows."""
    K1, K2, N, Ho, Wo = 32, 64, 96, 9, 7
    gen = torch.Generator().manual_seed(K1 + K2 + N)
    H2, W2 = 2 * Ho + 1, 2 * Wo
    a, b = torch.randn(B, K1, Ho, Wo, generator=gen), torch.randn(B, K2, H2, W2, generator=gen)
    wa, wb = torch.randn(N, K1, 1, 1, generator=gen) / (K1 + K2) ** 0.5, torch.randn(N, K2, 1, 1, generator=gen) / (K1 + K2) ** 0.5
    shift = torch.randn(N, generator=gen)
    ref = torch.relu(F.conv2d(a.double(), wa.double()) + F.conv2d(b.double(), wb.double(), stride=2)[:, :, :Ho, :Wo] + shift.double()[None, :, None, None])
    segs = Segs.make(B, [(Ho, Wo)])
    ab, bb = rows_of([a]).to(DEV), rows_of([b]).to(DEV)
    wp, sh = ops.pack_conv_weight(torch.cat([wa, wb], 1).to(DEV)), shift.to(DEV)

    def make(y):
        return ops.conv_call(ops.Rows(ab), segs, wp, y, Cin=K1, Cout=N, k=1, shift=sh, act=ACT_RELU, tile=tile, x2=ops.Rows(bb), x2_stride=2, x2_hw=(H2, W2))
    first = launch(make, segs.rows, N)
    close(first, rows_of([ref]), f"x2 tile {tile}")
    assert torch.equal(launch(make, segs.rows, N), first), "two runs differ"
    assert torch.equal(launch(make, segs.rows, N, BIG_CS), first), "the 32-bit arm and the pointer arm differ"


@pytest.mark.parametrize("tile", [2, 3, 4, 8, 9])
def test_row_group_statistics(tile):
    """gn_stats (the GNS instantiations; tiles 8, 9 GEMM-addressed): the stored output is bit for bit the one without statistics, every row's (sum, sum of
    squares) is written and is the sum over the stored values, nothing behind the table."""
    c = case_of("pw_pyramid", 64, "residual_relu")
    G = 8
    plain = c.launch(tile=tile)
    close(plain, c.ref, f"gn_stats tile {tile}")
    st = torch.full((c.rows + GUARD, G, 2), float("nan"), device=DEV)
    assert torch.equal(c.launch(tile=tile, gn_stats=st, gn_groups=G), plain), "the statistics changed the output"
    assert bool(torch.isnan(st[c.rows:]).all()), "wrote behind the statistics table"
    yv = plain.double().view(c.rows, G, 64 // G)
    np.testing.assert_allclose(st[:c.rows, :, 0].cpu().numpy(), yv.sum(-1).cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(st[:c.rows, :, 1].cpu().numpy(), (yv * yv).sum(-1).cpu().numpy(), rtol=1e-5, atol=1e-5)
    st2 = torch.full_like(st, float("nan"))
    c.launch(tile=tile, gn_stats=st2, gn_groups=G)
    assert torch.equal(st2[:c.rows], st[:c.rows]), "two runs differ"


@pytest.mark.parametrize("Cout", [64, 160])          # the gate's own tile choice: 64 x 64; 64 x 128 with a cut second column of tiles
def test_gated_loader(Cout):
    """gate + gate_b (the GATE instantiations): y = conv1x1(silu(x * a[img] + b[img])) + shift + residual over the pyramid."""
    Cin = 32
    gen = torch.Generator().manual_seed(Cout)
    segs = Segs.make(B, PYRAMID)
    xs = [torch.randn(B, Cin, h, w, generator=gen) for h, w in PYRAMID]
    wt = torch.randn(Cout, Cin, 1, 1, generator=gen) / Cin ** 0.5
    sf = torch.randn(Cout, generator=gen)
    coef = torch.stack([torch.rand(len(PYRAMID) * B, Cin, generator=gen) + 0.5, torch.randn(len(PYRAMID) * B, Cin, generator=gen)], 1).contiguous()
    rs = [torch.randn(B, Cout, h, w, generator=gen) for h, w in PYRAMID]
    ref = rows_of([F.conv2d(F.silu(x.double() * coef[lv * B:(lv + 1) * B, 0].double().view(B, Cin, 1, 1) + coef[lv * B:(lv + 1) * B, 1].double().view(B, Cin, 1, 1)),
                            wt.double(), sf.double()) + r.double() for lv, (x, r) in enumerate(zip(xs, rs))])
    xr, rr, cd = ops.Rows(rows_of(xs).to(DEV)), ops.Rows(rows_of(rs).to(DEV)), coef.to(DEV)
    wp, sh = ops.pack_conv_weight(wt.to(DEV)), sf.to(DEV)

    def make(y):
        return ops.conv_call(xr, segs, wp, y, Cin=Cin, Cout=Cout, k=1, shift=sh, res=rr, gate=cd[:, 0], gate_b=cd[:, 1], gate_act=ACT_SILU)
    first = launch(make, segs.rows, Cout)
    close(first, ref, f"gate Cout {Cout}")
    assert torch.equal(launch(make, segs.rows, Cout), first), "two runs differ"
    assert torch.equal(launch(make, segs.rows, Cout, BIG_CS), first), "the 32-bit arm and the pointer arm differ"


@pytest.mark.parametrize("tile", [4, 8, 9])
def test_upsampled_addend(tile):
    """res_up (the RUP instantiations) on an 8 x 6 map from 4 x 3: relu(conv) + Upsample(x2, nearest)(coarser), the addend read through pointers (its rows are not
    at a fixed stride), the stores through the descriptor."""
    Cin, Cout, H, W = 32, 64, 8, 6
    gen = torch.Generator().manual_seed(tile)
    segs = Segs.make(B, [(H, W)])
    x, up = torch.randn(B, Cin, H, W, generator=gen), torch.randn(B, Cout, H // 2, W // 2, generator=gen)
    wt = torch.randn(Cout, Cin, 1, 1, generator=gen) / Cin ** 0.5
    sc, sf = torch.rand(Cout, generator=gen) + 0.5, torch.randn(Cout, generator=gen) * 0.3
    ref = rows_of([F.relu(F.conv2d(x.double(), wt.double()) * sc.double()[None, :, None, None] + sf.double()[None, :, None, None])
                   + F.interpolate(up.double(), scale_factor=2, mode="nearest")])
    ub = torch.full((B * (H // 2) * (W // 2), Cout + 4), float("nan"), device=DEV)
    ub[:, 4:] = rows_of([up]).to(DEV)
    xr, wp, scd, sfd = ops.Rows(rows_of([x]).to(DEV)), ops.pack_conv_weight(wt.to(DEV)), sc.to(DEV), sf.to(DEV)

    def make(y):
        return ops.conv_call(xr, segs, wp, y, Cin=Cin, Cout=Cout, k=1, scale=scd, shift=sfd, act=ACT_RELU, tile=tile, res=ops.Rows(ub, 4, Cout), res_up=True)
    first = launch(make, segs.rows, Cout)
    close(first, ref, f"res_up tile {tile}")
    assert torch.equal(launch(make, segs.rows, Cout), first), "two runs differ"
    assert torch.equal(launch(make, segs.rows, Cout, BIG_CS), first), "the 32-bit arm and the pointer arm differ"
