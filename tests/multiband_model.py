"""Multi-band blending (--synopsis multiband, EU_SYN_MULTIBAND, eu_hip_blend_layers): the definition restated in
numpy, operation by operation, on top of the feather model's helpers (tests/feather_model.py: the facets' pixel, hit
and source coordinate, the ramp). The reference has no blending and the oracle knows none: this model is the yardstick
of tests/test_multiband_model.py (its own properties, no GPU) and tests/test_gpu_multiband.py (the device against
it, bit for bit). TEST CODE.

Every function takes `dtype`: float32 is the definition (include/eu_hip.h, eu_target::bands), float64 the
restatement of the same formulas that the float32 model is held to. Planes are (H, W) or (H, W, C) arrays.

    stage A   per facet the ray hits: q = e (alpha a: a * e), c = pixel (alpha: a > 1e-6 ? v / a : 0)
              Q_f = q on a hit else 0, M_f = Q_f > 0, X_f = M_f ? c : 0; qsum = sum Q_f, amax, count
              W_f = qsum > 0 ? Q_f / qsum : 0
    levels    w' = (w + 1) >> 1; L = bands clamped to L_max (min(w_L, h_L) >= 4; with wrap w % 2^L == 0); 0: min(L_max, 8)
    R         rows first: (((A[2i-2] + A[2i+2]) + 4 (A[2i-1] + A[2i+1])) + 6 A[2i]) / 16, then down the columns
    E         rows first: even ((A[i-1] + A[i+1]) + 6 A[i]) / 8, odd (A[i] + A[i+1]) / 2, then down the columns
    bands     where M^l > 0: B = X^l / M^l - E(X^{l+1}) / E(M^{l+1}) (0 unless E(M) > 0; top: X^L / M^L)
              num^l += W^l B, den^l += W^l, facets in job order
    collapse  O^L = num / den (0 unless den > 0), O^l = the same + E(O^{l+1})
    pixel     zeros where count == 0; O^0, with alpha O^0 * amax and alpha = amax
"""
import math

import numpy as np

import envutil_amd as ea
import feather_model as fm

F = np.float32
DEFAULT_BANDS = 8


def levels(w, h, bands=0):
    """L by the sizes alone: the pyramid levels above level 0 that keep min(w_L, h_L) >= 4"""
    want = bands if bands > 0 else DEFAULT_BANDS
    L = 0
    while L < want:
        w1, h1 = (w + 1) >> 1, (h + 1) >> 1
        if min(w1, h1) < 4:
            break
        w, h = w1, h1
        L += 1
    return L


def levels_of(width, height, bands=0, wrap=False):
    """the same with the wrap rule: width % 2^L == 0"""
    L = levels(width, height, bands)
    while wrap and L > 0 and width % (1 << L):
        L -= 1
    return L


def _index(k, n, wrap):
    return np.mod(k, n) if wrap else np.clip(k, 0, n - 1)


def _reduce_axis(A, axis, wrap):
    T = A.dtype.type
    n = A.shape[axis]
    i = 2 * np.arange((n + 1) >> 1)

    def g(o):
        return np.take(A, _index(i + o, n, wrap), axis=axis)
    return (((g(-2) + g(2)) + T(4) * (g(-1) + g(1))) + T(6) * g(0)) * T(0.0625)


def reduce(A, wrap=False):
    """R: along the rows (axis 1) first, then down the columns (axis 0), which always clamp"""
    return _reduce_axis(_reduce_axis(A, 1, wrap), 0, False)


def _expand_axis(A, nf, axis, wrap):
    T = A.dtype.type
    n = A.shape[axis]
    x = np.arange(nf)
    i = x >> 1

    def g(k):
        return np.take(A, _index(k, n, wrap), axis=axis)
    even = ((g(i - 1) + g(i + 1)) + T(6) * g(i)) * T(0.125)
    odd = (g(i) + g(i + 1)) * T(0.5)
    shape = [1] * A.ndim
    shape[axis] = nf
    return np.where((x & 1).reshape(shape) == 1, odd, even)


def expand(A, wf, hf, wrap=False):
    """E to the finer level's size wf x hf: along the rows first, then down the columns of the result"""
    return _expand_axis(_expand_axis(A, wf, 1, wrap), hf, 0, False)


def blend(X, Q, bands=0, wrap=False, dtype=np.float32):
    """everything behind stage A: X (N, H, W, C) and Q (N, H, W) -> O^0 (H, W, C)"""
    X, Q = np.asarray(X, dtype), np.asarray(Q, dtype)
    N, H, W = Q.shape
    L = levels_of(W, H, bands, wrap)
    zero = dtype(0)
    with np.errstate(all="ignore"):
        qsum = np.zeros((H, W), dtype)
        for f in range(N):
            qsum = qsum + Q[f]
        num, den = None, None
        for f in range(N):
            Ms = [np.where(Q[f] > 0, dtype(1), zero)]
            Ws = [np.where(qsum > 0, Q[f] / qsum, zero)]
            Xs = [np.where(Ms[0][:, :, None] > 0, X[f], zero)]
            for l in range(L):
                Xs.append(reduce(Xs[l], wrap))
                Ms.append(reduce(Ms[l], wrap))
                Ws.append(reduce(Ws[l], wrap))
            if num is None:
                num = [np.zeros(x.shape, dtype) for x in Xs]
                den = [np.zeros(m.shape, dtype) for m in Ms]
            for l in range(L + 1):
                m = Ms[l]
                B = Xs[l] / m[:, :, None]
                if l < L:
                    hf, wf = m.shape
                    em = expand(Ms[l + 1], wf, hf, wrap)
                    ex = expand(Xs[l + 1], wf, hf, wrap)
                    B = B - np.where(em[:, :, None] > 0, ex / em[:, :, None], zero)
                on = m > 0
                num[l] = np.where(on[:, :, None], num[l] + Ws[l][:, :, None] * B, num[l])
                den[l] = np.where(on, den[l] + Ws[l], den[l])
        O = None
        for l in range(L, -1, -1):
            o = np.where(den[l][:, :, None] > 0, num[l] / den[l][:, :, None], zero)
            if O is not None:
                hf, wf = den[l].shape
                o = o + expand(O, wf, hf, wrap)
            O = o
    return O.astype(dtype)


def blend_layers(colour, weight, bands=0, wrap=False, dtype=np.float32):
    """eu_hip_blend_layers: colour plays c, weight plays Q (what is not positive counts as 0); every pixel is O^0"""
    colour, weight = np.asarray(colour, dtype), np.asarray(weight, dtype)
    Q = np.where(weight > 0, weight, dtype(0))
    X = np.where(Q[..., None] > 0, colour, dtype(0))
    return blend(X, Q, bands, wrap, dtype)


def stage_a(facets, nch, width_px=0.0):
    """the layers of feather_model's per-facet arrays, float32: X (N, H, W, ncol), Q (N, H, W), amax, count"""
    shape = facets[0]["hit"].shape
    alpha = nch in (2, 4)
    ncol = nch - 1 if alpha else nch
    X = np.zeros((len(facets),) + shape + (ncol,), np.float32)
    Q = np.zeros((len(facets),) + shape, np.float32)
    amax = np.zeros(shape, np.float32)
    count = np.zeros(shape, np.int32)
    with np.errstate(all="ignore"):
        for f, fc in enumerate(facets):
            hit = np.asarray(fc["hit"], bool)
            v = fm.f32(fc["pixel"])
            e = fm.edge_weight(fc["sx"], fc["sy"], fc["win"], fc["border"], width_px)
            if alpha:
                a = v[:, :, nch - 1]
                q = fm.f32(a * e)
                c = np.where((a > fm.ALPHA_GATE)[:, :, None], fm.f32(v[:, :, :ncol] / a[:, :, None]), F(0))
                amax = np.where(hit, np.maximum(amax, a), amax)
            else:
                q, c = e, v
            Q[f] = np.where(hit, q, F(0))
            X[f] = np.where((Q[f] > 0)[:, :, None], c, F(0))
            count = count + hit
    return X, Q, amax, count


def multiband(facets, nch, width_px=0.0, bands=0, wrap=False, dtype=np.float32, details=False):
    """the frame from feather_model's per-facet arrays (feather() there documents them)"""
    X, Q, amax, count = stage_a(facets, nch, width_px)
    O = blend(X, Q, bands, wrap, dtype)
    out = np.zeros(count.shape + (nch,), dtype)
    ncol = O.shape[2]
    if nch in (2, 4):
        out[:, :, :ncol] = O * amax.astype(dtype)[:, :, None]
        out[:, :, ncol] = amax
    else:
        out[:] = O
    out[count == 0] = 0
    return (out, count) if details else out


def wraps(args):
    """column indices wrap: a spherical or cylindrical target of 360 degrees"""
    return args.projection in (ea.SPHERICAL, ea.CYLINDRICAL) and abs(math.radians(args.hfov) - 2.0 * math.pi) < 1e-6


def model_frame(args, facets, nch, details=False, dtype=np.float32, **render_kw):
    """the multiband frame of the job `args` over `facets` (feather_model.Facet objects), through the single-facet stages"""
    arrays = [fm.facet_arrays(args, f, nch, **render_kw) for f in facets]
    return multiband(arrays, nch, args.feather, args.bands, wraps(args), dtype, details)


def model_frame_at_rays(args, facets, gs, gws, nch, dtype=np.float32):
    """the same through the rays (feather_model.model_frame_at_rays; no twining: the library refuses it). Needs a device."""
    rays = [fm.stepper_rays(args, f) for f in facets]
    arrays = [fm.arrays_at_rays(r[0], f, g, gw, nch) for r, f, g, gw in zip(rays, facets, gs, gws)]
    return multiband(arrays, nch, args.feather, args.bands, wraps(args), dtype)


# ---- the pictures both test files blend (eu_hip_blend_layers) ---------------------------------------------------
# (width, height, layers, channels): the sizes the pyramid's edges show at - L_max 0, odd halving at every level,
# wrapped columns (64 x 6 has L_max 0, so 64 x 16 and 40 x 32 are added: L = 2, and 3 with 40 % 8 == 0), holes,
# more than one LDS tile each way
SIZES = [(4, 4, 2, 1), (5, 3, 2, 1), (9, 7, 3, 3), (64, 6, 2, 3), (33, 17, 4, 4), (130, 70, 2, 3), (64, 16, 2, 3), (40, 32, 3, 2)]


def setting(w, h):
    """(bands, wrap) of a size"""
    return (3, True) if (w, h) in ((64, 6), (64, 16), (40, 32)) else (0, False)


def pictures(w, h, n, c, seed=7):
    """random pictures with holes in the weights, a column no layer covers and (n > 2) a layer without weight"""
    rng = np.random.default_rng(seed + w * 131 + h)
    colour = rng.uniform(0.0, 1.0, (n, h, w, c)).astype(np.float32)
    weight = rng.uniform(0.05, 1.0, (n, h, w)).astype(np.float32)
    weight[rng.uniform(size=weight.shape) < 0.2] = 0.0
    weight[:, :, w // 3] = 0.0
    if n > 2:
        weight[n - 1] = 0.0
    return colour, weight
