"""Numpy restatement of vjf_kstep_score (include/vjf_hip.h, "Scoring predictions") in any dtype: from every row t of a filtered
record the mean map x <- x + Phi([x, u]) w_mean is rolled h = 1 .. K steps from mu[t] and compared with mu[t + h] and, through the
decoder, with y[t + h]; sums over the valid (t, b) per horizon and column.

`ordered=True` adds the terms in the order the library states: the record flattened to starts r = t B + b, tiles of 16 consecutive
starts, per tile the valid starts' terms in start order in the working dtype, every term rounded on its own, then the tiles' partials
in tile order in float64.  Otherwise numpy's own sum in the working dtype (what the fp64 reference uses)."""
import numpy as np

from oracle import vjf_oracle as orc

TILE = 16
ETA_MAX = 10.0


def _get(st, k):
    return st[k] if isinstance(st, dict) else getattr(st, k)


def mean_step(st, x, u, dt):
    """x + Phi([x, u]) w_mean for rows x (N, xdim), u (N, udim) or None."""
    c, lw, w = (np.asarray(_get(st, k), dt) for k in ("centroid", "logwidth", "w_mean"))
    feat = orc.rbf(orc.nonecat(x, u), c, np.exp(lw))
    return (x + feat @ w.reshape(c.shape[0], -1)).astype(dt)


def predictions(st, mu, u, K, dtype=np.float64):
    """pred (K, T, B, xdim): pred[h - 1, t] = xh_h from mu[t] where t + h <= T - 1, NaN elsewhere."""
    dt = dtype
    mu = np.asarray(mu, dt)
    T, B, dout = mu.shape
    u = None if u is None or np.shape(u)[-1] == 0 else np.asarray(u, dt)
    pred = np.full((K, T, B, dout), np.nan, dt)
    xh = mu.copy()
    for h in range(1, K + 1):
        m = T - h                                          # origins 0 .. m - 1 are valid at horizon h
        if m <= 0:
            break
        un = None if u is None else u[h:T].reshape(m * B, -1)          # origin t at step h reads u[t + h]
        xh = mean_step(st, xh[:m].reshape(m * B, dout), un, dt).reshape(m, B, dout)
        pred[h - 1, :m] = xh
    return pred


def fold(terms, ordered):
    """Sum over the rows of `terms` (starts in start order, columns): numpy's sum in the terms' dtype, or the stated order."""
    terms = np.asarray(terms)
    if terms.shape[0] == 0:
        return np.zeros(terms.shape[1], np.float64)
    if not ordered:
        return terms.sum(0, dtype=terms.dtype).astype(np.float64)
    nt = -(-terms.shape[0] // TILE)
    pad = np.zeros((nt * TILE, terms.shape[1]), terms.dtype)
    pad[:terms.shape[0]] = terms
    pad = pad.reshape(nt, TILE, -1)
    acc = np.zeros((nt, terms.shape[1]), terms.dtype)
    for b in range(TILE):                                  # start order inside a tile, every addition rounded
        acc = acc + pad[:, b]
    return np.cumsum(acc.astype(np.float64), axis=0)[-1]   # tile order, float64


def sq_terms(a, t):
    e = a - t                                              # (three roundings per term: the difference, its square, the sum)
    return e * e


def poisson_terms(eta, y):
    ec = np.minimum(eta, eta.dtype.type(ETA_MAX))
    return np.exp(ec) - y * ec


def sums_from_pred(pred, mu, ordered=True):
    """(sse_x, base_x) (K + 1, xdim) float64 from predictions and the record, in their dtype."""
    K, T, B, dout = pred.shape
    sse, base = np.zeros((K + 1, dout)), np.zeros((K + 1, dout))
    flat = lambda a: a.reshape(-1, a.shape[-1])            # noqa: E731
    for h in range(0, min(K, T - 1) + 1):
        m = T - h
        xh = mu[:m] if h == 0 else pred[h - 1, :m]
        sse[h] = fold(sq_terms(flat(xh), flat(mu[h:])), ordered)
        base[h] = fold(sq_terms(flat(mu[:m]), flat(mu[h:])), ordered)
    return sse, base


def score(st, mu, y=None, u=None, K=8, *, poisson=False, dtype=np.float64, ordered=False):
    """dict(n, sse_x, base_x, sse_y, base_y, pred): the sums (K + 1, dim) as float64, computed in `dtype`."""
    dt = dtype
    mu = np.asarray(mu, dt)
    T, B, dout = mu.shape
    pred = predictions(st, mu, u, K, dt)
    out = {"n": np.maximum(T - np.arange(K + 1), 0) * B, "pred": pred, "sse_y": None, "base_y": None}
    out["sse_x"], out["base_x"] = sums_from_pred(pred, mu, ordered)
    if y is not None:
        y = np.asarray(y, dt)
        W, b = np.asarray(_get(st, "dec_W"), dt), np.asarray(_get(st, "dec_b"), dt)
        dy = W.shape[0]
        dec = lambda x: (x @ W.T + b).astype(dt)           # noqa: E731
        term = poisson_terms if poisson else sq_terms
        sse, base = np.zeros((K + 1, dy)), np.zeros((K + 1, dy))
        for h in range(0, min(K, T - 1) + 1):
            m = T - h
            xh = mu[:m] if h == 0 else pred[h - 1, :m]
            tgt = y[h:].reshape(m * B, dy)
            sse[h] = fold(term(dec(xh.reshape(m * B, dout)), tgt), ordered)
            base[h] = fold(term(dec(mu[:m].reshape(m * B, dout)), tgt), ordered)
        out["sse_y"], out["base_y"] = sse, base
    return out
