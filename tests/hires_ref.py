"""An independent numpy restatement of the hires fix's four tap conventions, and the float64 application of given
tap tables.  No code of the product is used here.

    taps(mode, n_in, n_out)            -> (idx int64 [n_out, T], w float64 [n_out, T])
    resample_f64(x, iy, wy, ix, wx)    -> (y, S): y = the separable sum in float64, S = sum |wy| |wx| |x| per output

nearest-exact, bilinear and bicubic follow torch.nn.functional.interpolate(align_corners=False); lanczos3 follows Pillow's
Image.resize(..., LANCZOS) for upscaling (filter scale 1).
"""
import math

import numpy as np

MODES = ("nearest-exact", "bilinear", "bicubic", "lanczos3")
TAPS = {"nearest-exact": 1, "bilinear": 2, "bicubic": 4, "lanczos3": 7}

# (H, W) -> (Ho, Wo) of the CPU tests; the GPU tests add their tile-edge cases
SHAPES = [((1, 1), (3, 3)), ((2, 3), (8, 9)), ((5, 7), (9, 15)), ((8, 8), (12, 12)), ((8, 8), (16, 16)), ((8, 16), (20, 24)),
          ((8, 8), (8, 8)), ((64, 64), (96, 96))]


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos3(x):
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def taps(mode, n_in, n_out):
    T = TAPS[mode]
    idx = np.zeros((n_out, T), dtype=np.int64)
    w = np.zeros((n_out, T), dtype=np.float64)
    s = float(n_in) / float(n_out)
    for o in range(n_out):
        if mode == "nearest-exact":
            idx[o, 0] = min(int(math.floor((o + 0.5) * n_in / n_out)), n_in - 1)
            w[o, 0] = 1.0
        elif mode == "bilinear":
            c = max((o + 0.5) * s - 0.5, 0.0)
            i0 = int(math.floor(c))
            lam = c - i0
            idx[o] = (min(i0, n_in - 1), min(i0 + 1, n_in - 1))
            w[o] = (1.0 - lam, lam)
        elif mode == "bicubic":
            A = -0.75
            c = (o + 0.5) * s - 0.5
            i0 = int(math.floor(c))
            t = c - math.floor(c)

            def near(x):      # |x| <= 1
                return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

            def far(x):       # 1 < |x| < 2
                return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
            idx[o] = [min(max(i0 - 1 + k, 0), n_in - 1) for k in range(4)]
            w[o] = (far(t + 1.0), near(t), near(1.0 - t), far((1.0 - t) + 1.0))
        elif mode == "lanczos3":
            c = (o + 0.5) * s
            lo = max(int(c - 3.0 + 0.5), 0)
            hi = min(int(c + 3.0 + 0.5), n_in)
            n = hi - lo
            assert 1 <= n <= 7
            raw = [_lanczos3((k + lo) - c + 0.5) for k in range(n)]
            tot = 0.0
            for v in raw:
                tot += v
            for k in range(7):
                idx[o, k] = lo + min(k, n - 1)
                w[o, k] = raw[k] / tot if k < n else 0.0
        else:
            raise ValueError(mode)
    return idx, w


def resample_f64(x, iy, wy, ix, wx):
    """x [..., H, W]; iy / wy [Ho, Ty], ix / wx [Wo, Tx] -> (y, S) float64 [..., Ho, Wo]."""
    x = np.asarray(x, dtype=np.float64)
    iy, ix = np.asarray(iy, dtype=np.int64), np.asarray(ix, dtype=np.int64)
    wy, wx = np.asarray(wy, dtype=np.float64), np.asarray(wx, dtype=np.float64)

    def apply(v, wyy, wxx):
        h = (v[..., :, ix] * wxx).sum(axis=-1)                                   # [..., H, Wo]
        return (h[..., iy, :] * wyy[:, :, None]).sum(axis=-2)                    # [..., Ho, Ty, Wo] -> [..., Ho, Wo]
    return apply(x, wy, wx), apply(np.abs(x), np.abs(wy), np.abs(wx))
