"""Random isometries for the TSI stage — mirror of the reference's ``attack/ISO/isometry_init.py`` (same names and
signatures). Everything is float64 numpy on the host, and the angles come from the GLOBAL numpy generator, three (or four)
one-element ``np.random.uniform`` draws in the reference's order, so a seeded run draws the same matrices bit for bit.
"""
import numpy as np


def _angles(a, b):
    """Three angles, one draw each from [a[i], b[i]) (isometry_init.py:6-8)."""
    return [np.random.uniform(a[i], b[i], 1)[0] for i in range(3)]


def _axis(t1, t2):
    """The unit vector the reference builds from two angles (isometry_init.py:38,71,84)."""
    return np.array([np.sin(t1), np.cos(t1) * np.sin(t2), np.cos(t1) * np.cos(t2)])


def _r_z(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])


def rotation_xyz(a=np.zeros(3), b=2 * np.pi * np.ones(3)):
    """r_z r_y r_x with the reference's sign conventions (isometry_init.py:4-28) — the matrix TSI draws."""
    tx, ty, tz = _angles(a, b)
    cx, sx = np.cos(tx), np.sin(tx)
    cy, sy = np.cos(ty), np.sin(ty)
    r_x = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    r_y = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return np.dot(np.dot(_r_z(tz), r_y), r_x)


def rotation_axis_angle(a=np.zeros(3), b=2 * np.pi * np.ones(3)):
    """Rodrigues' formula about the axis of the first two angles; the rotation angle is a FOURTH draw from the third
    interval, after a third angle that is drawn and not used (isometry_init.py:31-46)."""
    t = _angles(a, b)
    u = _axis(t[0], t[1])
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    theta = np.random.uniform(a[2], b[2], 1)
    return np.identity(3) + np.sin(theta) * K + (1 - np.cos(theta)) * np.dot(K, K)


def rotation(a=np.zeros(3), b=2 * np.pi * np.ones(3)):
    """The closed-form Euler product of isometry_init.py:49-61."""
    t1, t2, t3 = _angles(a, b)
    c1, s1, c2, s2, c3, s3 = np.cos(t1), np.sin(t1), np.cos(t2), np.sin(t2), np.cos(t3), np.sin(t3)
    return np.array([[c1 * c3 - c2 * s1 * s3, -c2 * c3 * s1 - c1 * s3, s1 * s2],
                     [c3 * s1 + c1 * c2 * s3, c1 * c2 * c3 - s1 * s3, -c1 * s2],
                     [s2 * s3, c3 * s2, c2]])


def reflection(a=np.zeros(3), b=2 * np.pi * np.ones(3)):
    """I - 2 u^T u: the reflection in the plane through the origin with normal u (isometry_init.py:64-74)."""
    t = _angles(a, b)
    u = _axis(t[0], t[1])[None, :]
    return np.identity(3) - 2 * np.dot(u.transpose(), u)


def ref_rot(a=np.zeros(3), b=2 * np.pi * np.ones(3)):
    """The reflection above followed by a rotation about z by the third angle (isometry_init.py:77-92)."""
    t = _angles(a, b)
    u = _axis(t[0], t[1])[None, :]
    return np.dot(_r_z(t[2]), np.identity(3) - 2 * np.dot(u.transpose(), u))
