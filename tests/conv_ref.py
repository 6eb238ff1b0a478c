"""float64 reference of the dense convolution layer and the geometry table of the conv geometry tests
(test_conv_geometry_cpu.py, test_conv_geometry_gpu.py).  Plain torch on the CPU, no project code.

  forward(x, w, ...)      act(conv2d(x, w, stride, pad, dil) * scale + shift + res), NCHW float64
  grads(x, w, gy, ...)    dX, dW, d shift, d res of sum(forward * gy) through float64 autograd
  dgrad / wgrad           the same dX / dW in closed form (a transposed conv; a product over the unfolded input)
  h16                     an operand rounded to f16, then float64: the f16-operand variants are forward(h16(x), h16(w), ...) and so on
  to_rows / from_rows     NCHW <-> [B*H*W, C] rows;  pyr_to_rows / pyr_from_rows: the same over a list of levels (level-major, the library's layout)

Filters may be rectangular (w [Cout, Cin, KH, KW]); stride / pad / dil are ints or (h, w) pairs, as torch takes them."""
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------------ layouts
def to_rows(t: torch.Tensor) -> torch.Tensor:
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def from_rows(r: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    return r.reshape(B, H, W, r.shape[1]).permute(0, 3, 1, 2).contiguous()


def pyr_to_rows(maps: Sequence[torch.Tensor]) -> torch.Tensor:
    return torch.cat([to_rows(t) for t in maps], 0)


def pyr_from_rows(r: torch.Tensor, B: int, hw: Sequence[Tuple[int, int]]) -> List[torch.Tensor]:
    out, m = [], 0
    for h, w in hw:
        out.append(from_rows(r[m:m + B * h * w], B, h, w))
        m += B * h * w
    assert m == r.shape[0], "rows do not match the level list"
    return out


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_hw(H: int, W: int, kh: int, kw: int, stride, pad, dil) -> Tuple[int, int]:
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(pad), _pair(dil)
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def h16(t: torch.Tensor) -> torch.Tensor:
    """The operand as an f16 kernel sees it: rounded to f16 once (from fp32), arithmetic in float64 from there."""
    return t.float().half().double()


# ---------------------------------------------------------------------------------------------------- the layer
def _act(v: torch.Tensor, act: str) -> torch.Tensor:
    return {"none": lambda t: t, "relu": F.relu}[act](v)


def forward(x, w, stride=1, pad=0, dil=1, scale=None, shift=None, res=None, act: str = "none") -> torch.Tensor:
    y = F.conv2d(x.double(), w.double(), None, stride, pad, dil)
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    return _act(y, act)


class Grads(NamedTuple):
    y: torch.Tensor
    dx: torch.Tensor
    dw: torch.Tensor
    dshift: Optional[torch.Tensor]
    dres: Optional[torch.Tensor]


def grads(x, w, gy, stride=1, pad=0, dil=1, scale=None, shift=None, res=None, act: str = "none") -> Grads:
    """Forward and the gradients of sum(forward * gy) through float64 autograd."""
    x = x.double().clone().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    shift = shift.double().clone().requires_grad_(True) if shift is not None else None
    res = res.double().clone().requires_grad_(True) if res is not None else None
    y = forward(x, w, stride, pad, dil, scale, shift, res, act)
    (y * gy.double()).sum().backward()
    return Grads(y.detach(), x.grad, w.grad, shift.grad if shift is not None else None, res.grad if res is not None else None)


def dgrad(gy, w, in_hw: Tuple[int, int], stride=1, pad=0, dil=1) -> torch.Tensor:
    """dX of conv2d(x, w) for the upstream gradient gy, in closed form: the unpadded transposed conv is the gradient of the zero-padded input; the input is
    its window [pad, pad + H) x [pad, pad + W), zero where no window of the conv reached (rows / columns past the last window)."""
    H, W = in_hw
    (ph, pw) = _pair(pad)
    full = F.conv_transpose2d(gy.double(), w.double(), None, _pair(stride), 0, 0, 1, _pair(dil))
    full = F.pad(full, (0, max(0, pw + W - full.shape[3]), 0, max(0, ph + H - full.shape[2])))
    return full[:, :, ph:ph + H, pw:pw + W].contiguous()


def wgrad(x, gy, khw: Tuple[int, int], stride=1, pad=0, dil=1) -> torch.Tensor:
    """dW of conv2d(x, w) in closed form: dW[o, c, r, q] = sum over (n, i, j) of gy[n, o, i, j] * x[n, c, s*i - p + d*r, s*j - p + d*q]."""
    kh, kw = khw
    cols = F.unfold(x.double(), (kh, kw), _pair(dil), _pair(pad), _pair(stride))          # [B, C*kh*kw, L]
    g = gy.double().reshape(gy.shape[0], gy.shape[1], -1)                                  # [B, O, L]
    return torch.einsum("bol,bkl->ok", g, cols).reshape(gy.shape[1], x.shape[1], kh, kw)


# ------------------------------------------------------------------------------------------- the geometry table
class Geom(NamedTuple):
    gid: str                    # row of the table ("10a", "10b": its two even kernels; "14a".."14d": the rectangular filters)
    kh: int
    kw: int
    stride: int
    pad: int                    # one symmetric padding, rows and columns alike: what the kernels take
    dil: int
    H: int
    W: int
    widths: Tuple[Tuple[int, int], ...]     # (Cin, Cout) pairs this geometry runs at
    pyramid: bool = False       # also over the two levels (H, W), (ceil(H/2), ceil(W/2))
    why: str = ""

    @property
    def square(self) -> bool:
        return self.kh == self.kw

    def levels(self, pyramid: bool = False):
        return [(self.H, self.W), (-(-self.H // 2), -(-self.W // 2))] if pyramid else [(self.H, self.W)]


BATCH = 2
# Cin in {32, 96} (+ 64: a K-tile of 64 channels, + 40 at the ops level: a partial 32-channel chunk); Cout in {8, 36, 64, 160}: the 32-wide tile, a width
# with Cout % 32 != 0, one full tile, two tiles with a ragged second.  Two or three pairs per geometry, chosen so that every width meets every kernel size.
GEOMS = (
    Geom("1", 3, 3, 1, 0, 1, 9, 11, ((96, 64), (32, 36), (64, 160)), True, "'valid': the output is smaller than the input"),
    Geom("2", 3, 3, 1, 2, 1, 6, 7, ((32, 64), (96, 8)), False, "'full' padding, pad = k - 1"),
    Geom("3", 1, 1, 1, 1, 1, 7, 9, ((32, 64), (96, 36), (64, 160)), False, "a padded 1x1 is not GEMM-addressed"),
    Geom("4", 5, 5, 1, 2, 1, 9, 8, ((32, 160), (96, 36), (64, 64), (40, 36)), True, "25 taps"),
    Geom("5", 5, 5, 2, 2, 1, 11, 14, ((32, 64), (96, 8)), False, "strided 5x5, odd and even sizes"),
    Geom("6", 7, 7, 2, 3, 1, 13, 10, ((32, 36), (64, 64)), False, "a generic 7x7, M = 2*7*5"),
    Geom("7", 3, 3, 3, 1, 1, 12, 11, ((32, 64), (96, 160)), False, "stride 3: input row 11 is read by no window"),
    Geom("8", 3, 3, 1, 3, 3, 8, 9, ((32, 64), (96, 36), (64, 160)), True, "dilation 3, 'same'"),
    Geom("9", 3, 3, 2, 2, 2, 9, 9, ((32, 8), (96, 64)), False, "dilated and strided"),
    Geom("10a", 2, 2, 2, 0, 1, 8, 10, ((32, 64), (64, 36)), False, "even kernel 2x2"),
    Geom("10b", 4, 4, 2, 1, 1, 10, 8, ((96, 64), (32, 160)), False, "even kernel 4x4"),
    Geom("10c", 2, 2, 2, 0, 1, 9, 11, ((32, 64),), False, "2x2 stride 2 on odd sizes: input row 8 and column 10 are read by no window (a strided data gradient the kernels take)"),
    Geom("11", 3, 3, 2, 0, 1, 9, 12, ((32, 36), (96, 64)), False, "strided 'valid'"),
    Geom("12", 3, 3, 1, 4, 1, 5, 6, ((32, 64), (96, 160)), False, "windows entirely inside the padding; pad' < 0 for the data gradient"),
    Geom("13", 5, 5, 1, 2, 1, 2, 3, ((32, 8), (96, 64)), False, "a map smaller than the filter"),
    Geom("14a", 1, 3, 1, 0, 1, 7, 9, ((32, 64), (40, 36)), False, "KH != KW: 1x3"),
    Geom("14b", 1, 3, 1, 1, 1, 7, 9, ((96, 36),), False, "KH != KW: 1x3, padded (rows too)"),
    Geom("14c", 3, 1, 1, 0, 1, 7, 9, ((32, 160), (40, 36)), False, "KH != KW: 3x1"),
    Geom("14d", 2, 1, 1, 0, 1, 7, 9, ((96, 64),), False, "KH != KW: 2x1"),
    Geom("15", 3, 3, 1, 1, 1, 13, 10, ((32, 8), (96, 160), (64, 64), (40, 36)), True, "the tested twin, M = 260: a 128- and a 256-row tile boundary"),
)


class Case(NamedTuple):
    g: Geom
    Cin: int
    Cout: int
    pyramid: bool

    @property
    def id(self) -> str:
        g = self.g
        return f"g{g.gid}-{g.kh}x{g.kw}s{g.stride}p{g.pad}d{g.dil}-{self.Cin}to{self.Cout}" + ("-pyr" if self.pyramid else "")

    @property
    def levels(self):
        return self.g.levels(self.pyramid)

    def out_levels(self):
        g = self.g
        return [out_hw(h, w, g.kh, g.kw, g.stride, g.pad, g.dil) for h, w in self.levels]


def cases(square_only: bool = False, cin32: bool = False, cout4: bool = True) -> List[Case]:
    """Every (geometry, width pair) of the table, and for the pyramid geometries their first width pair over two levels as well.
    square_only: without the rectangular filters; cin32: without the Cin = 40 pairs (the nodes and the HIP weight packers take Cin % 32 == 0)."""
    out = []
    for g in GEOMS:
        if square_only and not g.square:
            continue
        pairs = [p for p in g.widths if not (cin32 and p[0] % 32)]
        out += [Case(g, ci, co, False) for ci, co in pairs]
        if g.pyramid:
            out.append(Case(g, pairs[0][0], pairs[0][1], True))
    return out


def seed_of(c: Case) -> int:
    g = c.g
    return (((g.kh * 7 + g.kw) * 5 + g.stride) * 5 + g.pad) * 1009 + g.dil * 101 + c.Cin * 3 + c.Cout + (17 if c.pyramid else 0)


def make_inputs(c: Case, gen: Optional[torch.Generator] = None):
    """Seeded fp32 inputs of a case: per level x [B, Cin, H, W], gy and res [B, Cout, Ho, Wo] ~ N(0, 1); w ~ N(0, 1 / (Cin*KH*KW)) so that outputs have unit
    scale (a dropped tap moves an output by ~ 1 / sqrt(taps)); scale in [0.5, 1.5), shift ~ N(0, 1)."""
    gen = gen or torch.Generator().manual_seed(seed_of(c))
    g = c.g
    xs = [torch.randn(BATCH, c.Cin, h, w, generator=gen) for h, w in c.levels]
    wt = torch.randn(c.Cout, c.Cin, g.kh, g.kw, generator=gen) / math.sqrt(c.Cin * g.kh * g.kw)
    scale = torch.rand(c.Cout, generator=gen) + 0.5
    shift = torch.randn(c.Cout, generator=gen)
    ress = [torch.randn(BATCH, c.Cout, h, w, generator=gen) for h, w in c.out_levels()]
    gys = [torch.randn(BATCH, c.Cout, h, w, generator=gen) for h, w in c.out_levels()]
    return xs, wt, scale, shift, ress, gys
