"""The output pass of the F(4x4) Winograd kernel (fd_conv_wino4.hip): the per-workgroup tile table its threads read their tile from, and the 32-bit
addressing of its stores and residual loads -- at the smallest shapes at which either can go wrong (ragged pyramids, a dead and a cut cout block, dilation 2
on an odd map, every epilogue variant, channel views, every launch form).  Every case is checked against an fp64 F.conv2d reference at the bound of
test_layers_gpu.test_conv3x3_winograd_f4x4, and bit for bit between two runs, the one-launch and the sliced form, the one-launch and the uncut persistent form."""
import pytest
import torch
import torch.nn.functional as F

from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd._lib import ACT_EXP, ACT_NONE, ACT_RELU, Segs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8                       # rows of NaN in front of and behind every output view: a padding tile that stored anything would land there (or in a neighbour's row)
PYRAMID = [(9, 7), (5, 6)]      # 2 images: 12 + 8 tiles -- one M tile whose second half holds 4 tiles and 12 padding tiles, two levels inside one half

# name -> (batch, levels, Cin, Cout, dilation)
GEOMS = {
    "pyramid_cout40": (2, PYRAMID, 16, 40),           # the second 32-cout block is cut at 40 by nn < Cout
    "pyramid_cout72": (2, PYRAMID, 16, 72),           # a second cout tile with one live block (and one dead block of waves)
    "dil2_odd_map": (5, [(7, 9)], 32, 72),            # four parity classes of 4 x 5, 3 x 5, 4 x 4, 3 x 4 pixels: tiles past the sub-grid edge; 40 tiles = two M tiles
}
DIL = {"pyramid_cout40": 1, "pyramid_cout72": 1, "dil2_odd_map": 2}
# name -> (act, act_c0, per-level parameter, residual, ReLU-mask residual)
EPILOGUES = {
    "relu_all": (ACT_RELU, 0, False, False, False),            # fast path
    "relu_from_c20": (ACT_RELU, 20, False, False, False),      # act_c0 inside the first cout tile: general path there, fast path in the second tile
    "scale_exp": (ACT_EXP, 4, True, False, False),             # a different seg_param per level
    "residual": (ACT_RELU, 0, False, True, False),
    "relu_mask": (ACT_NONE, 0, False, True, True),             # the data-gradient epilogue
}
PRM = [1.2, 0.9]


class Case:
    """Inputs, the fp64 reference and the one-launch result of one (geometry, epilogue): computed once, shared by the tests, never modified."""

    def __init__(self, geom, epi, Cin=None, Cout=None):
        B, hw, cin, cout = GEOMS[geom]
        self.B, self.hw, self.Cin, self.Cout, self.dil = B, hw, Cin or cin, Cout or cout, DIL[geom]
        self.act, self.act_c0, self.per_level, self.use_res, self.mask = EPILOGUES[epi]
        Cin, Cout, dil = self.Cin, self.Cout, self.dil
        gen = torch.Generator().manual_seed(1000 + 7 * Cin + Cout + len(geom) + len(epi))
        self.segs = Segs.make(B, hw)
        rows = self.segs.rows
        xs = [torch.randn(B, Cin, h, w, generator=gen) for h, w in hw]
        wt = torch.randn(Cout, Cin, 3, 3, generator=gen) / (Cin * 9) ** 0.5
        sc, sf = torch.rand(Cout, generator=gen) + 0.5, torch.randn(Cout, generator=gen) * 0.1
        rs = [torch.randn(B, Cout, h, w, generator=gen) for h, w in hw]
        self.ref = []
        for lv, (x, r) in enumerate(zip(xs, rs)):
            y = F.conv2d(x.double(), wt.double(), None, 1, dil, dil) * sc.double()[None, :, None, None] + sf.double()[None, :, None, None]
            if self.use_res:
                y = torch.where(r.double() > 0, y, torch.zeros_like(y)) if self.mask else y + r.double()
            if self.act == ACT_EXP:
                y = torch.cat([y[:, :4], torch.exp(y[:, 4:] * PRM[lv])], 1)
            elif self.act == ACT_RELU:
                y = torch.cat([y[:, :self.act_c0], F.relu(y[:, self.act_c0:])], 1)
            self.ref.append(y.float())
        xb = torch.full((rows, Cin + 8), float("nan"), device=DEV)
        xb[:, 4:4 + Cin] = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, Cin) for t in xs]).to(DEV)
        rb = torch.full((rows, Cout + 4), float("nan"), device=DEV)
        rb[:, 4:] = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, Cout) for t in rs]).to(DEV)
        self.x, self.wp = ops.Rows(xb, 4, Cin), ops.pack_conv_weight_wino4(wt.to(DEV))
        self.kw = dict(Cin=Cin, Cout=Cout, k=3, pad=dil, dil=dil, scale=sc.to(DEV), shift=sf.to(DEV), res=ops.Rows(rb, 4, Cout) if self.use_res else None,
                       res_mask=self.mask, act=self.act, act_c0=self.act_c0, seg_param=PRM[:len(hw)] if self.per_level else None, tile=_lib.WINO4_TILE)
        self.first = self.launch()

    def out(self, cs=None):
        """A NaN-filled buffer with GUARD rows around a [rows, Cout] view at channel 4 of `cs` channels."""
        cs = cs or self.Cout + 8
        buf = torch.full((self.segs.rows + 2 * GUARD, cs), float("nan"), device=DEV)
        return buf, ops.Rows(buf[GUARD:GUARD + self.segs.rows], 4, self.Cout)

    def call(self, y, **more):
        return ops.conv_call(self.x, self.segs, self.wp, y, **{**self.kw, **more})

    def launch(self, form=None, **more):
        """Run one form of the layer into a fresh NaN buffer; returns the [rows, Cout] result after checking that nothing else was written."""
        buf, y = self.out()
        run = self.call(y, **more)
        for q in (form(run) if form else [run]):
            q()
        torch.cuda.synchronize()
        got = y.tensor()
        outside = torch.ones_like(buf, dtype=torch.bool)
        outside[GUARD:GUARD + self.segs.rows, 4:4 + self.Cout] = False
        assert bool(torch.isnan(buf[outside]).all()), "wrote outside its channel view / rows"
        assert not bool(torch.isnan(got).any()), "an output pixel was never written"
        return got.clone()

    def check_ref(self, got, tag=""):
        got = got.cpu()
        for i, ((h, w), r) in enumerate(zip(self.hw, self.ref)):
            g = got[self.segs.m_start[i]:self.segs.m_start[i + 1]].reshape(self.B, h, w, self.Cout).permute(0, 3, 1, 2)
            scale = float(r.abs().max()) + 1.0
            err = (g - r).abs()
            print(f"{tag} level {i}: max err {float(err.max()):.3e} mean {float(err.mean()):.3e} scale {scale:.3f}")
            assert float(err.max()) < 4e-5 * scale and float(err.mean()) < 2e-6 * scale, (tag, i, float(err.max()), float(err.mean()), scale)


_cases = {}


def case_of(geom, epi, **kw):
    key = (geom, epi, tuple(sorted(kw.items())))
    if key not in _cases:
        _cases[key] = Case(geom, epi, **kw)
    return _cases[key]


def two_slices_reversed(run):
    total, _ = ops.conv_workgroups(run)
    cut = max(8, (total // 2) // 8 * 8)
    parts = [ops.conv_wg_slice(run, 0, cut, tag=1)] + ([ops.conv_wg_slice(run, cut, total - cut, tag=0)] if total > cut else [])
    return list(reversed(parts))


@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("geom", list(GEOMS))
def test_every_launch_form_of_every_epilogue(geom, epi):
    """One launch against fp64; two runs, the grid as two slices in reverse order and the persistent form without a cut item (8 workgroups: the one of an XCD
    walks all its items, rewriting the tile table per segment) bit for bit the same."""
    c = case_of(geom, epi)
    c.check_ref(c.first, f"{geom}/{epi}")
    assert torch.equal(c.launch(), c.first), "two runs differ"
    assert torch.equal(c.launch(two_slices_reversed), c.first), "the sliced form differs from the one launch"
    ws = ops.sk_workspace(8, DEV)
    assert torch.equal(c.launch(sk_wgs=8, workspace=ws), c.first), "the uncut persistent form differs from the one launch"
    assert int(ws[:2048].view(torch.int32).abs().sum()) == 0, "a slot flag / queue head was left non-zero"


@pytest.mark.parametrize("geom,Cin", [("pyramid_cout40", 32), ("dil2_odd_map", 32)])
def test_split_k(geom, Cin):
    """Split-K 2: raw partial outputs through the same output pass into the workspace (the slice offset folded into the resource's base), the combine launch
    applies the epilogue.  Same products in another summation order: the fp64 bound, and half of it against the one launch."""
    c = case_of(geom, "residual", Cin=Cin)
    c.check_ref(c.first, f"{geom}/one launch")
    ws = torch.full((2 * c.segs.rows * c.Cout + 64,), float("nan"), device=DEV)
    got = c.launch(ksplit=2, workspace=ws)
    c.check_ref(got, f"{geom}/split-K")
    assert torch.equal(c.launch(ksplit=2, workspace=ws), got), "two split-K runs differ"
    assert bool(torch.isnan(ws[2 * c.segs.rows * c.Cout:]).all()), "wrote behind the two slabs"
    assert float((got - c.first).abs().max()) < 2e-5 * (float(c.first.abs().max()) + 1.0)


def test_persistent_form_with_a_cut_item():
    """16 workgroups on one M tile x three cout tiles: XCD 0 queues items 0, 1 whole and item 2 as two pieces -- both its workgroups run two segments (the table
    is rewritten), one finishes the cut item from the other's slot.  Uncut items bit for bit the one launch, the cut item within the bounds of the persistent
    form's own test; identical from run to run."""
    c = case_of("pyramid_cout40", "residual", Cin=64, Cout=136)
    c.check_ref(c.first, "one launch")
    ws = ops.sk_workspace(16, DEV)
    got = c.launch(sk_wgs=16, workspace=ws)
    assert int(ws[:2048].view(torch.int32).abs().sum()) == 0, "a slot flag / queue head was left non-zero"
    c.check_ref(got, "persistent, cut")
    assert torch.equal(got[:, :128], c.first[:, :128]), "an uncut item differs from the one launch"
    assert float((got - c.first).abs().max()) < 1e-5 * (float(c.first.abs().max()) + 1.0)
    assert torch.equal(c.launch(sk_wgs=16, workspace=ws), got), "two runs differ"


def test_view_too_large_for_32_bit_offsets():
    """An output view of more than 3 GiB (few rows, a huge row stride) takes the output pass's 64-bit addressing: the same bits as the compact view, nothing
    written outside."""
    c = case_of("pyramid_cout72", "residual")
    cs = 4_400_000                                   # 186 rows: 3.27 GB, under the entry point's 2^31 elements
    assert (c.segs.rows - 1) * cs * 4 >= 0xC0000000 and c.segs.rows * cs < 2 ** 31
    buf = torch.full((c.segs.rows, cs), float("nan"), device=DEV)
    y = ops.Rows(buf, cs - c.Cout - 4, c.Cout)
    c.call(y)()
    torch.cuda.synchronize()
    assert torch.equal(y.tensor(), c.first)
    assert int(torch.isnan(buf).sum()) == buf.numel() - c.first.numel(), "wrote outside its channel view"
    del buf, y
    torch.cuda.empty_cache()
