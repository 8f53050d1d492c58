"""The device-side draw of the EOT loop's tables (pc3d_eot_draw_f32) restated on the CPU from the text of include/pc3d.h:
numpy only, uint64 arithmetic (which wraps mod 2^64)."""
import numpy as np

_U = np.uint64
G = _U(0x9E3779B97F4A7C15)
TWO_M53 = 2.0 ** -53


def mix64(z):
    """The splitmix64 finaliser on a uint64 scalar or array."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def stream(seed, n, e):
    """s of (seed, n, e): seed an int64 (negative values count as their two's complement)."""
    with np.errstate(over="ignore"):
        return mix64(_U(int(seed) & 0xFFFFFFFFFFFFFFFF) + G * (_U(16) * _U(int(n)) + _U(int(e)) + _U(1)))


def theta_axis(seed, n, e):
    """(theta float64, case 0 / 1 / 2 / 3: rotation about z, x, y, or the identity)."""
    s = stream(seed, n, e)
    u = [int(mix64(s ^ _U(1 << (32 + j)))) for j in range(3)]
    rad = np.sqrt(-2.0 * np.log(float((u[0] >> 11) + 1) * TWO_M53))
    theta = 1e-2 * rad * np.cos(2.0 * np.pi * (float(u[1] >> 11) * TWO_M53))
    r = float(u[2] >> 11) * TWO_M53
    return float(theta), (0 if r < 0.2 else 1 if r < 0.4 else 2 if r < 0.6 else 3)


def rotation(seed, n, e):
    """rot float64 [3,3]: cos / sin in double, BEFORE the table's rounding to float32; the 0 and 1 entries exact."""
    theta, case = theta_axis(seed, n, e)
    c, s = np.cos(theta), np.sin(theta)
    if case == 0:
        return np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]], dtype=np.float64)
    if case == 1:
        return np.array([[1, 0, 0], [0, c, s], [0, -s, c]], dtype=np.float64)
    if case == 2:
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float64)
    return np.eye(3, dtype=np.float64)


def columns(seed, n, e, K):
    """idx int64 [K]: the columns of the K smallest keys among c = 1 .. 2K - 1, by ascending key."""
    s = stream(seed, n, e)
    c = np.arange(1, 2 * K, dtype=np.uint64)
    keys = (mix64(s ^ c) & ~_U(0x3FFF)) | c
    return (np.sort(keys)[:K] & _U(0x3FFF)).astype(np.int64)


def inverse(idx, K):
    """inv int32 [K,2]: the at most two positions j, ascending, with idx[j] mod K == i, else -1. Point i is drawn by the
    columns i and i + K only (column 0 is never drawn), each at most once."""
    pos = np.full(2 * K, -1, dtype=np.int64)
    pos[idx] = np.arange(K)
    a, b = pos[:K], pos[K:]
    both = (a >= 0) & (b >= 0)
    inv = np.empty((K, 2), dtype=np.int32)
    inv[:, 0] = np.where(both, np.minimum(a, b), np.maximum(a, b))
    inv[:, 1] = np.where(both, np.maximum(a, b), -1)
    return inv


def draw(seed, n, e, K):
    """(rot float64 [3,3], idx int64 [K], inv int32 [K,2]) of draw index n, view e."""
    idx = columns(seed, n, e, K)
    return rotation(seed, n, e), idx, inverse(idx, K)
