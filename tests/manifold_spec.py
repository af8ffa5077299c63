"""The three definitions csrc/manifold.hip implements, restated in numpy by brute force (full distance matrices, np.partition, the MMD formula), and the error
bounds its results are held to.  torch-fidelity is not installed where this package is developed: these restate its `calc_cdist_part(...).kthvalue(k + 1)`
(squared), `(dist <= radii).any(dim=1)` and the unbiased estimate of `polynomial_mmd` from their published form, and agreement with the library itself has not
been run.

The bounds are the standard ones for f64 dot products (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1): a sum of n products evaluated in
ANY order, each product and each sum rounded once (or fused, which only helps), is off by at most g(n) sum |a_f b_f| with g(n) = n u / (1 - n u), u = 2^-53.
Every bound below is doubled, as `fidelity_spec.isc_bound` is: it then covers the difference between any two such evaluations -- the kernel's and this file's
own."""
import numpy as np

U = 2.0 ** -53


def g(n):
    return n * U / (1 - n * U)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


# ---- squared distances, radii, membership -------------------------------------------------------------------------------------------------------
def dist2(a, b):
    """f64 [Na, Nb]: max(0, (|a_i|^2 + |b_j|^2) - 2 a_i.b_j)."""
    a, b = _f64(a), _f64(b)
    na, nb = (a * a).sum(axis=1), (b * b).sum(axis=1)
    return np.maximum((na[:, None] + nb[None, :]) - 2.0 * (a @ b.T), 0.0)


def dist2_bound(a, b):
    """e(i, j) >= |d2_kernel - d2_spec|.  The computed value is ((n_a + n_b)(1 + d1) - 2 G)(1 + d2) with three dot products of length F in some order: each
    exact product a_f b_f carries at most F + 2 rounding factors (F from its dot product, two from the two subtractions / additions; the factor 2 is exact),
    so the error is at most g(F + 2) (|a|^2 + |b|^2 + 2 sum_f |a_f b_f|); max(0, .) moves a value towards the exact one, which is >= 0.  Doubled (module
    docstring)."""
    a, b = np.abs(_f64(a)), np.abs(_f64(b))
    na, nb = (a * a).sum(axis=1), (b * b).sum(axis=1)
    return 2 * g(a.shape[1] + 2) * (na[:, None] + nb[None, :] + 2.0 * (a @ b.T))


def knn_radius(x, k):
    """f64 [N]: the (k + 1)-th smallest of d2(i, .) over all j, the self distance defined as 0."""
    d = dist2(x, x)
    np.fill_diagonal(d, 0.0)
    return np.partition(d, k, axis=1)[:, k]


def radius_bound(x):
    """E_i >= |radius2_kernel(i) - radius2_spec(i)|: an order statistic moves by at most the largest perturbation of its arguments (it is 1-Lipschitz in the
    sup norm), so E_i = max_j e(i, j)."""
    return dist2_bound(x, x).max(axis=1)


def manifold_member(q, r, radius2):
    """uint8 [Nq]: 1 where some j has d2(q_i, r_j) <= radius2[j]."""
    return (dist2(q, r) <= _f64(radius2)[None, :]).any(axis=1).astype(np.uint8)


def member_undecided(q, r, radius2, radius2_err):
    """bool [Nq]: the queries this file cannot decide.  Against ball j the kernel compares a distance within e(i, j) of the spec's with a radius within
    radius2_err[j] of the spec's: the pair is decided inside where d2 - radius2 < -(e + err), outside where d2 - radius2 > e + err.  A query is decided when
    one pair is decided inside (member) or every pair is decided outside (no member)."""
    margin = dist2(q, r) - _f64(radius2)[None, :]
    tol = dist2_bound(q, r) + _f64(radius2_err)[None, :]
    return ~((margin < -tol).any(axis=1) | (margin > tol).all(axis=1))


# ---- KID --------------------------------------------------------------------------------------------------------------------------------------------
def poly_kernel(gram, degree, gamma, coef0):
    base = gamma * gram + coef0
    p = base
    for _ in range(degree - 1):
        p = p * base
    return p


def kid_mmd2(x, y, idx1, idx2, degree=3, gamma=None, coef0=1.0):
    """f64 [S]: (sum_{i != j} K(x_i, x_j) + sum_{i != j} K(y_i, y_j)) / (m (m - 1)) - 2 sum_{i, j} K(x_i, y_j) / (m m) per subset, the diagonal left out by
    position."""
    x, y = _f64(x), _f64(y)
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    out = []
    for i1, i2 in zip(np.asarray(idx1), np.asarray(idx2)):
        a, b = x[i1], y[i2]
        m = len(i1)
        off = ~np.eye(m, dtype=bool)
        sxx = poly_kernel(a @ a.T, degree, gamma, coef0)[off].sum()
        syy = poly_kernel(b @ b.T, degree, gamma, coef0)[off].sum()
        sxy = poly_kernel(a @ b.T, degree, gamma, coef0).sum()
        out.append((sxx + syy) / (m * (m - 1)) - 2.0 * sxy / (m * m))
    return np.asarray(out, dtype=np.float64)


def _kernel_sum_bound(a, b, degree, gamma, coef0, off_diagonal):
    """(a bound on the error of sum K over the kept pairs in any order, sum |K| + that bound).
      G      the dot product: |dG| <= g(F) sum_f |a_f b_f| =: eg
      base   fl(fl(gamma G^) + coef0): the product is off by |gamma| eg and its own rounding, E1 = |gamma| eg (1 + u) + u |gamma G|; the sum adds one more
             rounding: db = E1 (1 + u) + u |base|
      power  |b^^d - b^d| <= d B^(d - 1) db with B = |base| + db (mean value theorem on [-B, B]), and the d - 1 products add g(d - 1) B^d
      sum    n terms in any order: g(n - 1) on the sum of the computed magnitudes."""
    f = a.shape[1]
    gram = a @ b.T
    eg = g(f) * (np.abs(a) @ np.abs(b).T)
    base = gamma * gram + coef0
    e1 = abs(gamma) * eg * (1 + U) + U * np.abs(gamma * gram)
    db = e1 * (1 + U) + U * np.abs(base)
    big = np.abs(base) + db
    dk = degree * big ** (degree - 1) * db + g(degree - 1) * big ** degree
    mag = big ** degree
    if off_diagonal:
        keep = ~np.eye(len(a), dtype=bool)
        dk, mag = dk[keep], mag[keep]
    err = dk.sum() + g(dk.size - 1) * mag.sum()
    return err, mag.sum()


def kid_bound(x, y, idx1, idx2, degree=3, gamma=None, coef0=1.0):
    """f64 [S] >= |mmd2_kernel - mmd2_spec|.  With the three sums' errors exx, eyy, exy and magnitudes Mxx, Myy, Mxy from `_kernel_sum_bound`:
    T1 = (Sxx + Syy) / (m (m - 1)) carries the sums' errors and two roundings (the addition, the division; m (m - 1) is exact), T2 = 2 Sxy / (m m) one (the
    factor 2 is exact), and the subtraction one more on |T1| + |T2|.  Doubled (module docstring)."""
    x, y = _f64(x), _f64(y)
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    out = []
    for i1, i2 in zip(np.asarray(idx1), np.asarray(idx2)):
        a, b = x[i1], y[i2]
        m = len(i1)
        exx, mxx = _kernel_sum_bound(a, a, degree, gamma, coef0, True)
        eyy, myy = _kernel_sum_bound(b, b, degree, gamma, coef0, True)
        exy, mxy = _kernel_sum_bound(a, b, degree, gamma, coef0, False)
        t1, t2 = (mxx + myy) / (m * (m - 1)), 2.0 * mxy / (m * m)
        e1 = (exx + eyy) / (m * (m - 1)) + g(2) * t1
        e2 = 2.0 * exy / (m * m) + g(1) * t2
        out.append(2 * (e1 + e2 + U * (t1 + t2 + e1 + e2)))
    return np.asarray(out, dtype=np.float64)


def kid_subset_tables(n1, n2, subsets, subset_size, rng_seed=0):
    rng = np.random.RandomState(rng_seed)
    t1, t2 = [], []
    for _ in range(subsets):
        t1.append(rng.choice(n1, subset_size, replace=False))
        t2.append(rng.choice(n2, subset_size, replace=False))
    return np.asarray(t1, dtype=np.int64), np.asarray(t2, dtype=np.int64)


def precision_recall(fake, real, k=3):
    """(precision, recall, f_score) as torch-fidelity's `prc`: fake rows inside the real rows' balls, real rows inside the fake rows' balls."""
    p = float(manifold_member(fake, real, knn_radius(real, k)).astype(np.float64).mean())
    r = float(manifold_member(real, fake, knn_radius(fake, k)).astype(np.float64).mean())
    return p, r, 2 * p * r / max(p + r, 1e-5)
