"""Host-side mirror of `spline_traj_optm.utils.utils` (utils/utils.py:3-19) on numpy arrays."""
import numpy as np


def global_to_frenet(p, p0, yaw):
    """Rotate p - p0 by -yaw (:3-8): row 0 is the longitudinal, row 1 the lateral coordinate.
    p, p0: shape (2,) or (2, ...); yaw broadcasts against the trailing axes."""
    d = np.asarray(p, dtype=np.float64) - np.asarray(p0, dtype=np.float64)
    d = d.reshape(2, *d.shape[1:]) if d.ndim > 1 else d.reshape(2)
    c, s = np.cos(-np.asarray(yaw, dtype=np.float64)), np.sin(-np.asarray(yaw, dtype=np.float64))
    return np.stack([c * d[0] - s * d[1], s * d[0] + c * d[1]])


def align_yaw(yaw1, yaw2):
    """yaw1 shifted by a multiple of 2 pi to within pi of yaw2 (:10-13)."""
    d = np.asarray(yaw1, dtype=np.float64) - yaw2
    return np.arctan2(np.sin(d), np.cos(d)) + yaw2


def align_abscissa(s1, s2, total_length):
    """s1 shifted by a multiple of total_length towards s2 (:15-19)."""
    s1 = np.asarray(s1, dtype=np.float64); s2 = np.asarray(s2, dtype=np.float64)
    k = np.abs(s2 - s1) + total_length / 2.0
    shift = k - np.fmod(np.abs(s2 - s1) + total_length / 2.0, total_length)
    return s1 + shift * np.sign(s2 - s1)
