"""The two definitions csrc/fidelity.hip implements, restated in numpy, and the error bound its Inception Score is held to.  torch-fidelity is not installed
where this package is developed: these restate its `interpolate_bilinear_2d_like_tensorflow1x` (align_corners=False) and `isc_features_to_metric` from their
published form, and agreement with the library itself has not been run."""
import math

import numpy as np

F32 = np.float32


def resize_tf1_bilinear(u8, size, nhwc=True):
    """uint8 [B, H, W, C] (nhwc) or [B, C, H, W] -> f32 [B, C, size, size]; every numpy operation below is one f32 operation, rounded once."""
    x = np.asarray(u8)
    x = (x.transpose(0, 3, 1, 2) if nhwc else x).astype(F32)
    h, w = x.shape[-2:]

    def taps(n_in):
        g = np.arange(size, dtype=F32) * F32(n_in / size)          # the double quotient rounded to f32, then an f32 product
        i0 = g.astype(np.int64)
        return i0, np.minimum(i0 + 1, n_in - 1), g - i0.astype(F32)
    y0, y1, dy = taps(h)
    x0, x1, dx = taps(w)
    dy, dx = dy.reshape(1, 1, size, 1), dx.reshape(1, 1, 1, size)
    r0, r1 = x[:, :, y0], x[:, :, y1]
    a, b, c, d = r0[..., x0], r0[..., x1], r1[..., x0], r1[..., x1]
    top = a + (b - a) * dx
    bot = c + (d - c) * dx
    out = ((top + (bot - top) * dy) - F32(128)) / F32(128)
    assert out.dtype == F32
    return out


def row_order(index, shuffle=True, rng_seed=0):
    """Position j of the scored sequence holds row row_order(...)[j]: ascending image index, then RandomState(rng_seed).permutation(N)."""
    order = np.argsort(np.asarray(index, dtype=np.int64), kind="stable")
    if shuffle:
        order = order[np.random.RandomState(rng_seed).permutation(len(order))]
    return order.astype(np.int64)


def split_bounds(n, splits):
    return [(k * n // splits, (k + 1) * n // splits) for k in range(splits)]


def inception_score(logits, order=None, splits=10):
    """f64, the reference's per-row KL form: exp(mean_j sum_c p_jc (log p_jc - log q_c)) per split -> f64 [splits]."""
    x = np.asarray(logits, dtype=np.float64)
    x = x if order is None else x[np.asarray(order)]
    m = x.max(axis=1, keepdims=True)
    logp = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
    p = np.exp(logp)
    out = []
    for j0, j1 in split_bounds(len(x), splits):
        pk, lk = p[j0:j1], logp[j0:j1]
        with np.errstate(divide="ignore", invalid="ignore"):
            kl = np.where(pk == 0.0, 0.0, pk * (lk - np.log(pk.mean(axis=0, keepdims=True))))      # a term with p == 0 adds 0
        out.append(np.exp(kl.sum(axis=1).mean()))
    return np.asarray(out, dtype=np.float64)


def isc_bound(logits, order=None, splits=10):
    """A first-order bound on |score - spec| / score for ANY order of the sums and either algebraic form -> f64 [splits].

    u = 2^-53 (one rounding); exp and log are taken as accurate to one ulp, 2 u relative.  C = classes, n_k the split's length, G = the largest gap
    max_c x - min_c x of a row, M = max |x|, L = log C.  The score is exp(kl), so its relative error is the absolute error of kl (+ 2 u for the exp).
      lse    x - m is rounded (u G), so each exp(x - m) is off by u G + 2 u relative; C positive terms summed in any order add (C - 1) u; the log adds 2 u L
             (|log s| <= L); m + log s is rounded, u |lse| <= u (M + L):                        d_lse <= u (C + G + 2 + 3 L + M)
      logp   x - lse rounded, |logp| <= G + L:                                                  d_lp  <= d_lse + u (G + L)
      p      exp of it:                                                                         relative d_lp + 2 u
      row    sum_c p logp: each term off by |p logp| (d_lp + 3 u) + p d_lp; sum_c |p logp| <= L (an entropy), sum_c p = 1; C terms in any order add
             (C - 1) u L:                                                                       d_row <= (1 + L) (d_lp + 3 u) + C u L
      A      mean of n_k rows, each <= L in size: n_k u L for the sum and the division:         d_A   <= d_row + (n_k + 1) u L
      q      mean of n_k values of p: relative d_lp + 2 u + n_k u =: r_q
      B      sum_c q log q: d(q log q) = (1 + log q) dq, plus 3 u on |q log q| for the log and the product; sum_c q |1 + log q| <= 1 + L; C terms add
             (C - 1) u L:                                                                       d_B   <= (1 + L) (r_q + 3 u) + C u L
      kl     A - B rounded, |kl| <= L:                                                          d_kl  <= d_A + d_B + u L
    The per-row KL form sum_c p (logp - log q) has the same terms (its weights sum_c p |logp - log q| average to at most 2 L over a split), so TWICE the
    total covers the difference between any two evaluations -- the kernel's and the spec's own.  With d_lp <= u (C + 2 G + M + 4 L + 2) that is
      2 u [ (1 + L) (2 (C + 2 G + M + 4 L + 6) + n_k) + (2 C + n_k + 2) L + 2 ]   (the last 2 u: the final exp),
    a multiple of 2^-53 (C + n_k)(1 + log C) plus the terms in G and M the subtractions bring.  Derived, not fitted; below 1e-9 at every size the tests use."""
    x = np.asarray(logits, dtype=np.float64)
    x = x if order is None else x[np.asarray(order)]
    n, c = x.shape
    u, L = 2.0 ** -53, math.log(c)
    out = []
    for j0, j1 in split_bounds(n, splits):
        xs = x[j0:j1]
        G, M, nk = float((xs.max(axis=1) - xs.min(axis=1)).max()), float(np.abs(xs).max()), j1 - j0
        out.append(2 * u * ((1 + L) * (2 * (c + 2 * G + M + 4 * L + 6) + nk) + (2 * c + nk + 2) * L + 2))
    return np.asarray(out, dtype=np.float64)


def fid_from_statistics(features, mu, sigma):
    """The Frechet distance between the features' own (mean, unbiased covariance) and (mu, sigma), f64, through the eigenvalues of the covariance product."""
    x = np.asarray(features, dtype=np.float64)
    m = x.mean(axis=0)
    s = np.cov(x, rowvar=False)
    ev = np.linalg.eigvals(s @ np.asarray(sigma, dtype=np.float64))
    d = m - np.asarray(mu, dtype=np.float64)
    return float(d @ d + np.trace(s) + np.trace(sigma) - 2 * np.sqrt(ev.astype(np.complex128)).real.sum())
