"""Host-side mirror of `spline_traj_optm.utils.integrator` (utils/integrator.py:4-19) on numpy arrays.

Both return the collocation DEFECT of the step x1 -> x2 over dt with a constant control u, after the heading
of x2 (component 2) has been aligned to that of x1.  x1, x2: rows of 5 (shape (5,), (1, 5) or (M, 5)); u (2,),
(1, 2) or (M, 2); dt scalar or (M,).  The result has the shape of x1 broadcast against x2.
"""
import numpy as np

from . import utils


def _rows(a, n):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(-1, n)


def _f(model, dynamics, x, u):
    return np.asarray(dynamics(model, x.T, u.T)).reshape(x.shape[1], -1).T


def _aligned(x1, x2):
    t = x2.copy()
    t[:, 2] = utils.align_yaw(t[:, 2], x1[:, 2])
    return t


def hermite_simpson(model, dynamics, x1, x2, u, dt):
    """Hermite-Simpson defect (:4-11)."""
    shape = np.broadcast(np.asarray(x1), np.asarray(x2)).shape
    x1 = _rows(x1, 5); x2 = _rows(x2, 5); u = _rows(u, 2); dt = np.reshape(np.asarray(dt, dtype=np.float64), (-1, 1))
    x1, x2 = np.broadcast_arrays(x1, x2)
    t = _aligned(x1, x2)
    f1 = _f(model, dynamics, x1, u); f2 = _f(model, dynamics, t, u)
    xm = 0.5 * (x1 + t) + (dt / 8.0) * (f1 - f2)
    fm = _f(model, dynamics, xm, u)
    return (x1 + (dt / 6.0) * (f1 + 4 * fm + f2) - t).reshape(shape)


def rk4(model, dynamics, x1, x2, u, dt):
    """Classical Runge-Kutta step minus the aligned end point (:13-19)."""
    shape = np.broadcast(np.asarray(x1), np.asarray(x2)).shape
    x1 = _rows(x1, 5); x2 = _rows(x2, 5); u = _rows(u, 2); dt = np.reshape(np.asarray(dt, dtype=np.float64), (-1, 1))
    x1, x2 = np.broadcast_arrays(x1, x2)
    t = _aligned(x1, x2)
    k1 = _f(model, dynamics, x1, u)
    k2 = _f(model, dynamics, x1 + dt / 2 * k1, u)
    k3 = _f(model, dynamics, x1 + dt / 2 * k2, u)
    k4 = _f(model, dynamics, x1 + dt * k3, u)
    return (x1 + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4) - t).reshape(shape)
