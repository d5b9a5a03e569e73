"""The packed-blob cases whose bytes tests/golden/blob_sha256.json pins (tests/test_blob_bytes_cpu.py
recomputes them, tools/blob_hashes.py writes the file).

Every host packer at the smallest, the default and the widest shapes plus the edges of its format,
on seeded normal weights with planted values that reach every branch of the element conversions.
The hash is over the whole buffer, pre-filled with 0xA5, so the zero padding is pinned too.
"""
from __future__ import annotations

import ctypes
import hashlib
import zlib

import numpy as np

POLICY_SHAPES = ((1, 2), (37, 6), (47, 12), (47, 2), (1, 12))  # (in, out)
POLICY_PRECISIONS = ("bf16", "f32", "f32x3")
VALUE_INS = (1, 37, 47)
CRITIC_INS = (1, 31, 32, 33, 99, 1539)  # 32: the bias column opens a second 32-column W1 chunk
ATTN_SHAPES = ((1, 0, 2), (3, 4, 6), (16, 5, 12))  # (K, Ms, out)
TOWER_PRECISIONS = ("bf16", "f32")

H = 256
EM = 32


def _bits(*words) -> np.ndarray:
    return np.array(words, np.uint32).view(np.float32)


# finite values every conversion takes: +-0; exact bf16 ties with an even (0x3f80|8000) and an odd
# (0x3f81|8000) kept bit, both signs, and their neighbours one f32 ulp off the tie; f32 subnormals;
# the exact f16 ties 1 + 2^-11 (even) and 1 + 3 2^-11 (odd)
FINITE = _bits(0x00000000, 0x80000000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F817FFF,
               0x00000001, 0x807FFFFF, 0x3F801000, 0x3F803000)
# bf16 and f32 blobs: quiet and signalling-pattern NaNs (the second has payload bits only below the
# bf16 cut), +-inf, and the largest f32 (rounds to bf16 inf)
NONFINITE = _bits(0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x7F7FFFFF)
# f32x3 (refuses what rounds past 65504): 65504, the last f32 below 65520 (rounds to 65504), -65504;
# the f16 subnormal range: 2^-24, the tie 2^-25 (to zero), one ulp above it (to 2^-24), one ulp below,
# the tie 3 2^-25 (to 2 2^-24), 1e-5, and either side of the smallest normal 2^-14
X3_EDGES = _bits(0x477FE000, 0x477FEFFF, 0xC77FE000, 0x33800000, 0x33000000, 0x33000001, 0x32FFFFFF, 0x33C00000,
                 0x3727C5AC, 0x38800000, 0x387FFFFF, 0xB87FFFFF)


def specials(precision: str) -> np.ndarray:
    return np.concatenate([FINITE, X3_EDGES if precision == "f32x3" else NONFINITE])


def _plant(a: np.ndarray, vals: np.ndarray, start: int) -> None:
    """vals at flat indices start, start + 7, ... (every planted array has >= 256 elements)."""
    flat = a.reshape(-1)
    assert start + 7 * len(vals) <= 256 <= flat.size
    for i, v in enumerate(vals):
        flat[start + 7 * i] = v


def normals(key: str, shapes, scales) -> list:
    """float32 normals from RandomState(crc32(key)): a frozen stream."""
    rng = np.random.RandomState(zlib.crc32(key.encode()))
    return [(rng.standard_normal(s) * sc).astype(np.float32) for s, sc in zip(shapes, scales)]


def mlp_weights(key: str, in_dim: int, out_dim: int, precision: str) -> list:
    """w1, b1, w2, b2, w3, b3 of a 256-256 tower; planted values in the four converted arrays."""
    a = normals(key, [(H, in_dim), (H,), (H, H), (H,), (out_dim, H), (out_dim,)], [0.2, 0.1, 0.06, 0.1, 0.06, 0.1])
    sp = specials(precision)
    for arr, start in ((a[0], 7), (a[1], 3), (a[2], 5), (a[4], 11)):
        _plant(arr, sp, start)
    return a


def attn_weights(key: str, ms: int, out_dim: int, precision: str) -> list:
    """swarm_attn_weights_t's fourteen arrays in field order.  The front end takes the finite planted
    values only (it is folded in float64 into every layer-1 row); the trunk takes them all."""
    in1 = 9 + EM + 4 * ms
    front = normals(key + "/front", [(EM, 4), (EM,), (EM, 9), (EM,), (3 * EM, EM), (3 * EM,), (EM, EM), (EM,)],
                    [0.3, 0.1, 0.3, 0.1, 0.2, 0.1, 0.2, 0.1])
    _plant(front[2], FINITE, 7)
    _plant(front[4], FINITE, 3)
    _plant(front[6], FINITE, 5)
    trunk = normals(key + "/trunk", [(H, in1), (H,), (H, H), (H,), (out_dim, H), (out_dim,)],
                    [0.2, 0.1, 0.06, 0.1, 0.06, 0.1])
    sp = specials(precision)
    for arr, start in ((trunk[0], 7), (trunk[1], 3), (trunk[2], 5), (trunk[4], 11)):
        _plant(arr, sp, start)
    return front + trunk


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _sha(nb: int, pack) -> str:
    assert nb > 0, nb
    buf = np.full(nb, 0xA5, np.uint8)
    assert pack(buf.ctypes.data_as(ctypes.c_void_p)) == 0
    return hashlib.sha256(buf.tobytes()).hexdigest()


def blob_hashes(lib, nat) -> dict:
    """{case key: SHA-256 of the packed blob} of every case, from the loaded library."""
    prec = {"bf16": nat.POLICY_BF16, "f32": nat.POLICY_F32, "f32x3": nat.POLICY_F32X3}
    out = {}
    for i, o in POLICY_SHAPES:
        for p in POLICY_PRECISIONS:
            key = f"policy/in{i}_out{o}/{p}"
            a = mlp_weights(key, i, o, p)
            out[key] = _sha(lib.swarm_policy_packed_bytes(i, o, prec[p]),
                            lambda dst: lib.swarm_policy_pack(i, o, prec[p], *map(_fp, a), dst))
    for name, ins in (("value", VALUE_INS), ("critic", CRITIC_INS)):
        nbytes, pack = getattr(lib, f"swarm_{name}_packed_bytes"), getattr(lib, f"swarm_{name}_pack")
        for i in ins:
            for p in TOWER_PRECISIONS:
                key = f"{name}/in{i}/{p}"
                a = mlp_weights(key, i, 1, p)
                out[key] = _sha(nbytes(i, prec[p]), lambda dst: pack(i, prec[p], *map(_fp, a), dst))
    for k, ms, o in ATTN_SHAPES:
        for p in TOWER_PRECISIONS:
            key = f"attn/k{k}_ms{ms}_out{o}/{p}"
            a = attn_weights(key, ms, o, p)
            w = nat.SwarmAttnWeights(*map(_fp, a))
            out[key] = _sha(lib.swarm_attn_policy_packed_bytes(k, ms, o, prec[p]),
                            lambda dst: lib.swarm_attn_policy_pack(k, ms, o, prec[p], ctypes.byref(w), dst))
    return out
