"""numpy restatement of the dropout definition of include/tribe_hip.h (tribe_dropout_apply), shared by the dropout tests.  It imports
no product code: the generator, the counter layout, the threshold and the scale are written out again here.

Element (r, c) of a logical [rows, dim] tensor has idx = r * dim + c; its word is word idx & 3 of Philox4x32-10 with counter
(lo32(idx >> 2), hi32(idx >> 2), lo32(site), hi32(site)) and key (lo32(seed), hi32(seed)); it is kept iff word >= trunc(p * 2^32);
kept values are multiplied by float32(1 / (1 - p)), dropped ones are +0.0."""

import numpy as np
import torch

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter: np.ndarray, key: np.ndarray) -> np.ndarray:
    """uint32 [..., 4] counters and uint32 [..., 2] keys (broadcast against each other) -> uint32 [..., 4]."""
    c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
    k = [np.asarray(key[..., i], dtype=np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _32) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(_W0)) & _MASK, (k[1] + np.uint64(_W1)) & _MASK]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def threshold(p: float) -> int:
    return int(p * 4294967296.0)


def scale(p: float) -> np.float32:
    return np.float32(1.0 / (1.0 - p))


def words(rows: int, dim: int, seed: int, site: int) -> np.ndarray:
    """uint32 [rows, dim]: the random word of every element."""
    n = rows * dim
    quads = (n + 3) // 4
    q = np.arange(quads, dtype=np.uint64)
    counter = np.empty((quads, 4), dtype=np.uint32)
    counter[:, 0] = (q & _MASK).astype(np.uint32)
    counter[:, 1] = (q >> _32).astype(np.uint32)
    counter[:, 2] = site & 0xFFFFFFFF
    counter[:, 3] = site >> 32
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    return philox4x32_10(counter, key).reshape(-1)[:n].reshape(rows, dim)


def keep_mask(rows: int, dim: int, p: float, seed: int, site: int) -> np.ndarray:
    """bool [rows, dim]: True where the element is kept."""
    return words(rows, dim, seed, site) >= np.uint32(threshold(p))


def expected(x: torch.Tensor, p: float, seed: int, site: int) -> torch.Tensor:
    """What tribe_dropout_apply makes of the CPU tensor x [rows, dim] (f32 or bf16): x.float() * scale rounded by torch's own cast
    where kept, +0.0 where dropped."""
    keep = torch.from_numpy(keep_mask(x.shape[0], x.shape[1], p, seed, site))
    y = (x.float() * torch.tensor(float(scale(p)), dtype=torch.float32)).to(x.dtype)
    return torch.where(keep, y, torch.zeros((), dtype=x.dtype))


def multiplier(rows: int, dim: int, p: float, seed: int, site: int) -> torch.Tensor:
    """float64 [rows, dim]: mask * scale, the factor a float64 composition multiplies by."""
    return torch.from_numpy(keep_mask(rows, dim, p, seed, site).astype(np.float64) * float(scale(p)))
