"""The reference of the tangent-dynamics tests (tests/test_tangent_ref.py, test_tangent_host.py, test_gpu_tangent.py): a numpy
restatement, in the caller's dtype, of what vjf_tangent_rollout computes, on the state arrays `oracle.vjf_oracle.forecast` uses (an
OracleState's centroid, logwidth, w_mean).

    f(x, u) = x + Phi([x, u]) w_mean                       the mean of RBFDS.forward(sampling=False)
    J(x, u) = I - w_mean^T G,  G[k, j] = phi_k (x_j - c_kj) / width_k^2
    J q     = q - w_mean^T s,  s_k = (phi_k / width_k^2)(x^T q - (C_x q)_k)

and one pass of modified Gram-Schmidt in column order (R_vv = |column v| > 0) every `qr_every` steps and behind the last step."""
import numpy as np

from oracle import vjf_oracle as orc


def step(s, x, u, Q):
    """x (B, xdim), u (B, udim) or None, Q (B, xdim, m)  ->  f(x, u) (B, xdim),  V = J(x, u) Q (B, xdim, m)."""
    xdim = x.shape[1]
    w = np.exp(s.logwidth)
    phi = orc.rbf(orc.nonecat(x, u), s.centroid, w)                 # (B, n)
    g = phi / (w * w)[None, :]
    xq = np.einsum("bj,bjv->bv", x, Q)                              # (B, m)
    cq = np.einsum("kj,bjv->bkv", s.centroid[:, :xdim], Q)          # (B, n, m)
    S = g[:, :, None] * (xq[:, None, :] - cq)
    V = Q - np.einsum("ki,bkv->biv", s.w_mean, S)
    return x + phi @ s.w_mean, V


def mgs(V):
    """One pass of modified Gram-Schmidt in column order on every (xdim, m) frame of V (B, xdim, m): Q, log R_vv (B, m)."""
    Q = np.array(V, copy=True)
    B, _, m = Q.shape
    logr = np.empty((B, m), Q.dtype)
    for v in range(m):
        r = np.sqrt(np.sum(Q[:, :, v] * Q[:, :, v], axis=1))
        logr[:, v] = np.log(r)
        Q[:, :, v] = Q[:, :, v] / r[:, None]
        for w in range(v + 1, m):
            dot = np.sum(Q[:, :, v] * Q[:, :, w], axis=1)
            Q[:, :, w] = Q[:, :, w] - dot[:, None] * Q[:, :, v]
    return Q, logr


def identity_frame(B, xdim, m, dtype):
    return np.broadcast_to(np.eye(xdim, m, dtype=dtype), (B, xdim, m)).copy()


def rollout(s, x0, u, q0, T, m, qr_every, lsum0=None):
    """(x (B, xdim), Q (B, xdim, m), lhist (ceil(T / qr_every), B, m), lsum (B, m)) after T steps from x0 / q0 (None: the first m
    columns of I); lsum0: sums to go on from.  qr_every = 0: never normalised (Q is the raw product, lhist is empty, lsum is lsum0)."""
    dt = s.dtype
    x = np.atleast_2d(np.asarray(x0, dt))
    B, xdim = x.shape
    Q = identity_frame(B, xdim, m, dt) if q0 is None else np.asarray(q0, dt).reshape(B, xdim, m).copy()
    lsum = np.zeros((B, m), dt) if lsum0 is None else np.asarray(lsum0, dt).copy()
    hist = []
    if T == 0 and qr_every > 0:
        Q, logr = mgs(Q)
        lsum = lsum + logr
    for t in range(T):
        x, Q = step(s, x, None if u is None else np.asarray(u[t], dt), Q)
        if qr_every > 0 and ((t + 1) % qr_every == 0 or t + 1 == T):
            Q, logr = mgs(Q)
            lsum = lsum + logr
            hist.append(logr)
    return x, Q, (np.stack(hist) if hist else np.zeros((0, B, m), dt)), lsum


def jacobian(s, x, u=None):
    """J[b, i, j] = d f_i / d x_j at x (B, xdim), u (B, udim) or None."""
    x = np.atleast_2d(np.asarray(x, s.dtype))
    return step(s, x, None if u is None else np.asarray(u, s.dtype), identity_frame(x.shape[0], x.shape[1], x.shape[1], s.dtype))[1]


def trajectory(s, x0, u, T):
    """x[0 .. T] of the mean map."""
    xs = [np.atleast_2d(np.asarray(x0, s.dtype))]
    for t in range(T):
        xs.append(step(s, xs[-1], None if u is None else np.asarray(u[t], s.dtype), np.zeros((xs[-1].shape[0], xs[-1].shape[1], 1), s.dtype))[0])
    return np.stack(xs)
