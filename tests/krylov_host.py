"""The three Krylov iterations of csrc/linalg.hip restated on the host (numpy / scipy), iterate by iterate.  A plain
helper module like mg_cycle_host.py: it uses nothing from the device.  Each iteration is written from its textbook
form plus the rules the header comments of csrc/linalg.hip state; the caller supplies the operator (a
`mg_cycle_host._Mat`, row mask applied: `masked`), the right-hand side, the start vector and the preconditioner.

bicgstab              right-preconditioned BiCGStab (van der Vorst): rhat = r0, and per iteration
                        phat = M^-1 p ; v = A phat ; alpha = rho / rhat.v  (0 when rhat.v = 0)
                        s = r - alpha v ; shat = M^-1 s ; t = A shat ; omega = t.s / t.t  (0 unless t.t > 0)
                        x += alpha phat + omega shat ; r = s - omega t
                      rho and |r|^2 of the new residual come from the five sums t.s, t.t, rhat.s, rhat.t, s.s:
                        rho = rhat.s - omega rhat.t ;  |r|^2 = max(s.s - 2 omega t.s + omega^2 t.t, 0)
                      The next direction p = r + (rho / rho_old) (alpha / omega) (p - omega v) -- unless the
                      recurrence has broken down: rho^2 <= 1e-16 |r|^2 |rhat|^2, rho_old = 0 or omega = 0.  Then it
                      restarts from the current residual: rhat = r, p = r, rho = |rhat|^2 = |r|^2.
pcg_jacobi            classic preconditioned CG, z = dinv r: alpha = r.z / p.Ap (0 when p.Ap = 0), beta = new r.z / old
                      r.z (0 when the old one is 0).
pcg_single_reduction  the Chronopoulos-Gear form: u = M^-1 r, w = A u, gamma = r.u, delta = w.u;
                        beta = gamma / gamma_old  (0 in the first iteration or when gamma_old = 0)
                        alpha = gamma / (delta - beta gamma / alpha_old)  (the correction is left out in the first
                        iteration and when alpha_old = 0; alpha = 0 when the denominator is 0)
                        p = u + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s
project_mean          (both CGs, the all-Neumann problem) the right-hand side is replaced by b - mean(b) before the
                      solve; nothing else is projected.

Row masks are part of the operator (`masked`): "identity" (the Newton systems of the momentum equation) replaces the
flagged rows by rows of the identity; "zero" (CG) zeroes the flagged rows, and the residual on them is zero whatever
the right-hand side holds there (`flags` of the CG functions).  Every direction then vanishes on the flagged dofs, so
the flagged columns act on the start vector alone -- which carries the boundary values -- and the iteration is the
one of the matrix with rows and columns removed.

Every function runs in the precision of the operator it is given (float64: scipy products; numpy.longdouble: dense
matrices or row sums on the CSR arrays, `mg_cycle_host._Mat`) and returns a `History`: x[j], res[j] (the recurrence
residual norm), the scalars of iteration j for j = 1 .. k under their names, r0 = |b - A x0| and bnorm = |b| (of the
projected right-hand side where there is a projection)."""
import numpy as np

from mg_cycle_host import LD, _Mat, rel  # noqa: F401  (rel: for the callers)

RESTART_THRESHOLD = 1e-16


def masked(A, flags, mode, dtype=np.float64):
    """the operator with its row mask as a _Mat of `dtype`: mode "identity" | "zero" | None; `flags` bool per row"""
    import scipy.sparse as sp
    A = sp.csr_matrix(A, dtype=np.float64)
    if mode is not None:
        flags = np.asarray(flags, dtype=bool)
        keep = sp.diags((~flags).astype(np.float64))
        A = keep @ A
        if mode == "identity":
            A = A + sp.diags(flags.astype(np.float64))
        else:
            assert mode == "zero"
        A = sp.csr_matrix(A)
        A.eliminate_zeros()
    A.sort_indices()
    return _Mat(A, dtype)


def jacobi(A, flags=None):
    """1 / diag in the precision of A, 1 on flagged rows (identity rows; rows of the zero mode carry no residual)"""
    d = A.diagonal()
    if flags is not None:
        d = np.where(np.asarray(flags, dtype=bool), A.dtype(1.0), d)
    return A.dtype(1.0) / d


class History:
    def __init__(self, names):
        self.x, self.res, self.r0, self.bnorm = [None], [None], None, None
        self.names = names
        for nme in names:
            setattr(self, nme, [None])

    def push(self, x, res, **scalars):
        assert set(scalars) == set(self.names)
        self.x.append(x.copy())
        self.res.append(res)
        for nme, v in scalars.items():
            getattr(self, nme).append(v)


def _norm(v):
    return np.sqrt(np.dot(v, v))


def _project(b, project_mean):
    return b - np.sum(b) / b.dtype.type(b.size) if project_mean else b


def _residual(A, b, x, flags):
    """b - A x; zero on the rows of a zero mask, whatever b holds there (|b| counts those entries all the same)"""
    r = b - A.dot(x)
    return r if flags is None else np.where(np.asarray(flags, dtype=bool), A.dtype(0.0), r)


def bicgstab(A, b, x0, apply_prec, k):
    """k iterations from x0; History with alpha, omega, rho (the rho the iteration ran with), restart (the iteration
    began with a restart) and the five sums ts, tt, rhs, rht, ss"""
    dt = A.dtype
    zero, one = dt(0.0), dt(1.0)
    b, x = np.asarray(b, dtype=dt), np.array(x0, dtype=dt)
    h = History(("alpha", "omega", "rho", "restart", "ts", "tt", "rhs", "rht", "ss"))
    r = b - A.dot(x)
    rhat = r.copy()
    rr = np.dot(r, r)
    rho, rhat2 = rr, rr
    rho_old = alpha = omega = one
    h.r0, h.bnorm = np.sqrt(rr), _norm(b)
    p = v = None
    for j in range(1, k + 1):
        restart = False
        if j == 1:
            p = r.copy()
        else:
            restart = bool(rho * rho <= dt(RESTART_THRESHOLD) * rr * rhat2 or rho_old == zero or omega == zero)
            if restart:
                rhat = r.copy()
                p = r.copy()
                rho = rhat2 = rr
            else:
                beta = (rho / rho_old) * (alpha / omega)
                p = r + beta * (p - omega * v)
        phat = apply_prec(p)
        v = A.dot(phat)
        rtv = np.dot(rhat, v)
        alpha = rho / rtv if rtv != zero else zero
        s = r - alpha * v
        shat = apply_prec(s)
        t = A.dot(shat)
        ts, tt, rhs, rht, ss = np.dot(t, s), np.dot(t, t), np.dot(rhat, s), np.dot(rhat, t), np.dot(s, s)
        omega = ts / tt if tt > zero else zero
        x = x + (alpha * phat + omega * shat)
        r = s - omega * t
        rho_old = rho
        rr = max(ss - dt(2.0) * omega * ts + omega * omega * tt, zero)
        rho = rhs - omega * rht
        h.push(x, np.sqrt(rr), alpha=alpha, omega=omega, rho=rho_old, restart=restart, ts=ts, tt=tt, rhs=rhs, rht=rht,
               ss=ss)
    h.rho_next = rho                                   # rhat.r of the last residual
    return h


def pcg_jacobi(A, b, x0, dinv, k, project_mean=False, flags=None):
    """k iterations of classic CG with z = dinv r; History with alpha, beta.  flags: the rows of the zero mask"""
    dt = A.dtype
    zero = dt(0.0)
    b = _project(np.asarray(b, dtype=dt), project_mean)
    x = np.array(x0, dtype=dt)
    dinv = np.asarray(dinv, dtype=dt)
    h = History(("alpha", "beta"))
    r = _residual(A, b, x, flags)
    z = dinv * r
    p = z.copy()
    rz = np.dot(r, z)
    h.r0, h.bnorm = _norm(r), _norm(b)
    for _ in range(k):
        q = A.dot(p)
        pq = np.dot(p, q)
        alpha = rz / pq if pq != zero else zero
        x = x + alpha * p
        r = r - alpha * q
        z = dinv * r
        rz_new = np.dot(r, z)
        beta = rz_new / rz if rz != zero else zero
        p = z + beta * p
        rz = rz_new
        h.push(x, _norm(r), alpha=alpha, beta=beta)
    return h


def pcg_single_reduction(A, b, x0, apply_prec, k, project_mean=False, flags=None):
    """k iterations of the Chronopoulos-Gear form; History with alpha, beta, gamma, delta.  flags: as in pcg_jacobi"""
    dt = A.dtype
    zero = dt(0.0)
    b = _project(np.asarray(b, dtype=dt), project_mean)
    x = np.array(x0, dtype=dt)
    h = History(("alpha", "beta", "gamma", "delta"))
    r = _residual(A, b, x, flags)
    h.r0, h.bnorm = _norm(r), _norm(b)
    u = apply_prec(r)
    w = A.dot(u)
    gamma, delta = np.dot(r, u), np.dot(w, u)
    gamma_old = alpha_old = zero
    p = s = None
    for j in range(1, k + 1):
        first = j == 1
        beta = zero if (first or gamma_old == zero) else gamma / gamma_old
        den = delta
        if not first and alpha_old != zero:
            den = den - beta * gamma / alpha_old
        alpha = gamma / den if den != zero else zero
        p = u.copy() if first else u + beta * p
        s = w.copy() if first else w + beta * s
        x = x + alpha * p
        r = r - alpha * s
        h.push(x, _norm(r), alpha=alpha, beta=beta, gamma=gamma, delta=delta)
        gamma_old, alpha_old = gamma, alpha
        u = apply_prec(r)
        w = A.dot(u)
        gamma, delta = np.dot(r, u), np.dot(w, u)
    return h
