"""float64 restatement of the ResNet stem's weight gradient (fd_stem7x7_bwd_weight_nhwc4), for the tests:

    dW[co][ci][ky][kx] = scale[co] * sum over (n, oy, ox) of g[n][co][oy][ox] * x[n][ci][2 oy - 3 + ky][2 ox - 3 + kx],   g = dy, or dy * (y > 0)

with taps outside the image contributing zero; the result is torch's OIHW [64][3][7][7]."""
import numpy as np


def stem_wgrad_ref(x, dy, y=None, scale=None) -> np.ndarray:
    """x [N, 3, H, W], dy (and y) [N, Cout, H/2, W/2], scale [Cout] or None -> float64 [Cout, 3, 7, 7]."""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(dy, dtype=np.float64)
    if y is not None:
        g = g * (np.asarray(y) > 0)
    N, Ci, H, W = x.shape
    _, Co, Ho, Wo = g.shape
    assert H % 2 == 0 and W % 2 == 0 and (Ho, Wo) == (H // 2, W // 2)
    xp = np.zeros((N, Ci, H + 6, W + 6), dtype=np.float64)
    xp[:, :, 3:3 + H, 3:3 + W] = x
    dw = np.zeros((Co, Ci, 7, 7), dtype=np.float64)
    for ky in range(7):
        for kx in range(7):
            win = xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]            # x[n][ci][2 oy - 3 + ky][2 ox - 3 + kx]
            dw[:, :, ky, kx] = np.einsum("nohw,nchw->oc", g, win)
    if scale is not None:
        dw *= np.asarray(scale, dtype=np.float64).reshape(-1, 1, 1, 1)
    return dw
