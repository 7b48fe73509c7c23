"""Host-side mirror of `spline_traj_optm.models.dynamic_bicycle` (models/dynamic_bicycle.py:1-81) on numpy arrays.

Kinematic bicycle with slip angle at the centre of gravity: state (x, y, theta, delta, v), control (a, delta_dot).
The reference writes these on CasADi symbols; here they take numpy arrays whose LEADING axis is the component
(shape (5, ...) / (2, ...), or flat (5,) / (2,)), so they also evaluate many states at once.  The min-time NLP
built on them runs on the GPU (include/rl_mincurv.h: rl_bicycle_*); these functions are what the tests pin the
device functions and the bound callables of `set_up_bicycle_problem` to.
"""
import numpy as np


def dynamics(model_dict, x, u):
    """d/dt (x, y, theta, delta, v)  (:4-23).  beta = atan2(lr delta, L) is the slip angle at the CoG."""
    x = np.asarray(x, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    x = x.reshape(5, *x.shape[1:]) if x.ndim > 1 else x.reshape(5)
    theta, delta, v = x[2], x[3], x[4]
    a, delta_dot = u.reshape(2, *u.shape[1:])[0], u.reshape(2, *u.shape[1:])[1]
    lr, L = model_dict["lr"], model_dict["L"]
    beta = np.arctan2(lr * delta, L)
    omega = v * np.cos(beta) * np.tan(delta) / L
    return np.stack([v * np.cos(theta + beta), v * np.sin(theta + beta), omega, delta_dot * np.ones_like(omega),
                     a * np.ones_like(omega)])


def nx():
    return 5


def nu():
    return 2


def x_l(model_dict):
    """Lower state bounds (:34-36), a 1 x 5 row like the reference's DM(...).T."""
    return np.array([[-np.inf, -np.inf, -np.inf, -1.0 * model_dict["delta_max"], 0.0]])


def x_u(model_dict):
    """Upper state bounds (:39-42)."""
    return np.array([[np.inf, np.inf, np.inf, model_dict["delta_max"], model_dict["v_max"]]])


def u_l(model_dict):
    """Lower control bounds (:45-48): (a_lon_min, -delta_dot_max)."""
    return np.array([[model_dict["a_lon_min"], -1.0 * model_dict["delta_dot_max"]]])


def u_u(model_dict):
    """Upper control bounds (:51-54): (a_lon_max, delta_dot_max)."""
    return np.array([[model_dict["a_lon_max"], model_dict["delta_dot_max"]]])


def lat_acc(model_dict, x, u):
    """Yaw rate times the speed norm |(vx, vy)| (:65-67)."""
    f = dynamics(model_dict, x, u)
    return f[2] * np.sqrt(f[0] * f[0] + f[1] * f[1])


def lon_acc(model_dict, x, u):
    """The commanded acceleration (:70-71)."""
    u = np.asarray(u, dtype=np.float64)
    return u.reshape(2, *u.shape[1:])[0]
