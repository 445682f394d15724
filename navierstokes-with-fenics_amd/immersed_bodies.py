"""Immersed solid bodies in the IMEX pressure-correction step: Brinkman volume penalisation.

The momentum equation gains  (chi / eta) (u - u_s):  chi is the indicator of the solid (sharp, or smoothed over a
half width ``smoothing``), u_s(x) = U + W x (x - c) its rigid velocity and eta the permeability time scale.  The
device evaluates the term explicitly, as part of the extrapolated vector (``nsfem_set_bodies``, include/nsfem.h;
DESIGN.md 4o), so the matrices, the single CG solve and the one-launch lattice right-hand side stay untouched.  The
price is a bound on k / eta, ``stiff_step_bound``.

A body is a ``Ball`` (disc in 2D), an axis-aligned ``Box`` or a ``HalfSpace``; ``ImmersedBodies`` collects up to 16
of them with eta and the smoothing and goes to ``IMEXIPCSSolver.set_immersed_bodies``.  A body with ``motion`` (a
function t -> (centre, velocity, angular velocity)) is moved by the solver before every step.

Heated bodies: a body with a ``temperature`` T_s is thermal -- where a scalar is transported
(``BoussinesqIMEXSolver``) its equation gains (chi / eta_scalar) (T - T_s), evaluated explicitly inside the scalar
convection kernel (``nsfem_set_body_temperatures``) and bounded by the same ``stiff_step_bound`` on
k / eta_scalar.  A body without a temperature is thermally passive: the scalar passes through it as through fluid.
``IMEXIPCSSolver`` without a scalar ignores the temperatures.
"""
import math

import numpy as np

KIND_BALL, KIND_BOX, KIND_HALF_SPACE = 1, 2, 3
MAX_BODIES = 16


def _vector(name, value, dim=None):
    v = np.atleast_1d(np.asarray(value, dtype=np.float64)).ravel()
    if v.size not in ((2, 3) if dim is None else (dim, )) or not np.isfinite(v).all():
        raise ValueError("%s must be a finite vector of 2 or 3 numbers, got %r" % (name, value))
    return v


class _Body:
    kind = None

    def __init__(self, centre, size, velocity=None, angular=None, motion=None, temperature=None):
        self.centre = _vector("centre", centre)
        self.dim = self.centre.size
        self.size = self._check_size(size)
        self.velocity = np.zeros(self.dim) if velocity is None else _vector("velocity", velocity, self.dim)
        self.angular = self._check_angular(np.zeros(1 if self.dim == 2 else 3) if angular is None else angular)
        if motion is not None and not callable(motion):
            raise ValueError("motion must be a function t -> (centre, velocity, angular)")
        self.motion = motion
        if temperature is not None:
            temperature = float(temperature)
            if not math.isfinite(temperature):
                raise ValueError("temperature must be a finite number or None, got %r" % (temperature, ))
        #: T_s of a thermal body; None: thermally passive
        self.temperature = temperature

    def _check_angular(self, angular):
        w = np.atleast_1d(np.asarray(angular, dtype=np.float64)).ravel()
        if w.size != (1 if self.dim == 2 else 3) or not np.isfinite(w).all():
            raise ValueError("angular must be one finite number in 2D and three in 3D, got %r" % (angular, ))
        return w

    def at(self, t):
        """the pose at time t: the body itself without ``motion``, else a copy with its centre, velocity and angular
        velocity"""
        if self.motion is None:
            return self
        centre, velocity, angular = self.motion(float(t))
        moved = type(self)(centre, self.size if self.kind != KIND_BALL else self.size[0], velocity, angular,
                           temperature=self.temperature)
        if moved.dim != self.dim:
            raise ValueError("motion changed the dimension of the body")
        return moved

    def row(self):
        """(kind, centre, size, velocity, angular), the row ``NsfemContext.set_bodies`` takes"""
        return (self.kind, self.centre, self.size, self.velocity, self.angular)

    def velocity_at(self, X):
        """u_s at the points X [n, dim]"""
        r = np.asarray(X, dtype=np.float64) - self.centre
        if self.dim == 2:
            return self.velocity + self.angular[0] * np.stack([-r[:, 1], r[:, 0]], axis=1)
        return self.velocity + np.cross(self.angular, r)


class Ball(_Body):
    """|x - c| <= r (a disc in 2D)"""
    kind = KIND_BALL

    def _check_size(self, size):
        r = float(size)
        if not (math.isfinite(r) and r > 0.0):
            raise ValueError("Ball: the radius must be finite and > 0, got %r" % (size, ))
        return np.array([r])

    def distance(self, X):
        return np.linalg.norm(np.asarray(X, dtype=np.float64) - self.centre, axis=1) - self.size[0]


class Box(_Body):
    """|x_a - c_a| <= h_a: axis-aligned, half widths h"""
    kind = KIND_BOX

    def _check_size(self, size):
        h = _vector("half widths", size, self.dim)
        if not (h > 0.0).all():
            raise ValueError("Box: the half widths must be > 0, got %r" % (size, ))
        return h

    def distance(self, X):
        q = np.abs(np.asarray(X, dtype=np.float64) - self.centre) - self.size
        return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0)


class HalfSpace(_Body):
    """(x - c) . n <= 0 with the unit normal n pointing out of the solid"""
    kind = KIND_HALF_SPACE

    def _check_size(self, size):
        n = _vector("normal", size, self.dim)
        if abs(float(np.linalg.norm(n)) - 1.0) > 1e-12:
            raise ValueError("HalfSpace: the normal must have length 1, got %r" % (size, ))
        return n

    def distance(self, X):
        return (np.asarray(X, dtype=np.float64) - self.centre) @ self.size


def mask(distance, smoothing=0.0):
    """chi(d): 1 where d <= 0 for smoothing 0; else 1 for d <= -eps, 0 for d >= eps and
    0.5 (1 - d/eps - sin(pi d/eps)/pi) between"""
    d = np.asarray(distance, dtype=np.float64)
    if smoothing == 0.0:
        return (d <= 0.0).astype(np.float64)
    z = d / smoothing
    between = 0.5 * (1.0 - z - np.sin(np.pi * z) / np.pi)
    return np.where(d <= -smoothing, 1.0, np.where(d >= smoothing, 0.0, between))


class ImmersedBodies:
    """up to 16 bodies of one dimension, the penalisation parameter ``eta`` > 0 and the smoothing half width >= 0;
    ``eta_scalar`` > 0 is the eta_T of the thermal bodies (None: ``eta``)"""

    def __init__(self, bodies, eta, smoothing=0.0, eta_scalar=None):
        bodies = list(bodies)
        if not 1 <= len(bodies) <= MAX_BODIES:
            raise ValueError("ImmersedBodies: 1 to %d bodies, got %d" % (MAX_BODIES, len(bodies)))
        if not all(isinstance(b, _Body) for b in bodies) or len({b.dim for b in bodies}) != 1:
            raise ValueError("ImmersedBodies: bodies must be Ball, Box or HalfSpace objects of one dimension")
        eta, smoothing = float(eta), float(smoothing)
        if not (math.isfinite(eta) and eta > 0.0):
            raise ValueError("ImmersedBodies: eta must be finite and > 0, got %r" % (eta, ))
        if not (math.isfinite(smoothing) and smoothing >= 0.0):
            raise ValueError("ImmersedBodies: smoothing must be finite and >= 0, got %r" % (smoothing, ))
        eta_scalar = eta if eta_scalar is None else float(eta_scalar)
        if not (math.isfinite(eta_scalar) and eta_scalar > 0.0):
            raise ValueError("ImmersedBodies: eta_scalar must be finite and > 0, got %r" % (eta_scalar, ))
        self.bodies, self.eta, self.smoothing, self.eta_scalar = bodies, eta, smoothing, eta_scalar
        self.dim = bodies[0].dim

    @property
    def moving(self):
        return any(b.motion is not None for b in self.bodies)

    @property
    def thermal(self):
        """is any body thermal (has a temperature)?"""
        return any(b.temperature is not None for b in self.bodies)

    def temperatures(self):
        """(flags, values) of ``NsfemContext.set_body_temperatures``: flag 1 and T_s for a thermal body, 0 and 0.0
        for a passive one"""
        flags = np.array([0 if b.temperature is None else 1 for b in self.bodies], dtype=np.int32)
        values = np.array([0.0 if b.temperature is None else b.temperature for b in self.bodies])
        return flags, values

    def rows(self, t=None):
        """the rows of ``NsfemContext.set_bodies`` / ``move_bodies``, at time t where a body has a motion"""
        return [(b if t is None else b.at(t)).row() for b in self.bodies]

    def winner(self, X, t=None):
        """(chi, index) of the body that counts at the points X: the largest chi, the lowest index on ties"""
        chi = np.stack([mask((b if t is None else b.at(t)).distance(X), self.smoothing) for b in self.bodies])
        win = np.argmax(chi, axis=0)                      # (the first of equal maxima)
        return chi[win, np.arange(chi.shape[1])], win


def stiff_step_stable(alpha, beta, x):
    """do the roots of  alpha0 z^2 + alpha1 z + alpha2 + x (beta0 z + beta1)  lie in the closed unit disc (to 1e-12)?
    x = k / eta: one step of  u' = -u / eta  under the scheme alpha, beta does not grow.  One root solve."""
    p = [float(alpha[0]), float(alpha[1]) + x * float(beta[0]), float(alpha[2]) + x * float(beta[1])]
    while p and p[0] == 0.0:
        p = p[1:]
    roots = np.roots(p) if len(p) > 1 else np.zeros(0)
    return bool(np.all(np.abs(roots) <= 1.0 + 1e-12))


def stiff_step_bound(alpha, beta, tol=1e-9):
    """the largest x = k / eta for which ``stiff_step_stable`` holds: the stability limit of the explicit
    penalisation term where nothing else damps it.  Bisection on the scheme's own coefficients (about 70 root solves,
    half a millisecond); uniform steps give 4/3 for SBDF2, 1 for CNAB and mCNAB and 0 for CNLF (leapfrog is unstable
    for a damping term).  The result lies within ``tol`` BELOW the limit: to test one given k / eta, ask
    ``stiff_step_stable``."""
    def stable(x):
        return stiff_step_stable(alpha, beta, x)

    if not stable(0.0):
        return 0.0
    lo, hi = 0.0, 1.0
    while stable(hi):
        lo, hi = hi, 2.0 * hi
        if hi > 1.0e6:
            return math.inf
    while hi - lo > tol * max(1.0, hi):
        mid = 0.5 * (lo + hi)
        if stable(mid):
            lo = mid
        else:
            hi = mid
    return lo
