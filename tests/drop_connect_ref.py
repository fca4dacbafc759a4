"""numpy transcription of the stochastic-depth mask of csrc/bn.hip (k_bn_apply_drop; the formula is documented in
include/atomnas_hip.h) and of the key of the tail dropout (k_bn_act_pool), for the tests of the feature."""
import numpy as np

M64 = (1 << 64) - 1
STEP_MUL = 0x100000001B3
DROP_CONNECT_CONST = 0xD1B54A32D192ED03


def _u64(v):
    return np.asarray(v).astype(np.uint64)


def hash32(key):
    """upper word of the splitmix64 finaliser (hash32 of csrc/bn.hip); key: uint64 array"""
    with np.errstate(over="ignore"):
        k = _u64(key) + np.uint64(0x9E3779B97F4A7C15)
        k = (k ^ (k >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        k = (k ^ (k >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        k = k ^ (k >> np.uint64(31))
    return (k >> np.uint64(32)).astype(np.uint32)


def _base(seed, step):
    return np.uint64((int(seed) & M64) ^ ((int(step) * STEP_MUL) & M64))


def drop_connect_keys(seed, step, block_index, n):
    """uint64 keys of images n (array) of block `block_index` at step `step` (None: the kernel's step_ptr == NULL, step 0)"""
    step = 0 if step is None else step
    b = np.uint64(((int(block_index) << 40) & M64) ^ DROP_CONNECT_CONST)
    return _base(seed, step) ^ b ^ (_u64(n) << np.uint64(8))


def dropout_keys(seed, step, index):
    """uint64 keys of the tail dropout for the element indices n * C + c"""
    step = 0 if step is None else step
    return _base(seed, step) ^ (_u64(index) << np.uint64(20))


def uniform(keys):
    """the float32 value in [0, 1) a key is compared with the rate as"""
    return (hash32(keys) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_mask(seed, step, block_index, N, p):
    """uint8 [N]: 1 where image n keeps its branch"""
    u = uniform(drop_connect_keys(seed, step, block_index, np.arange(N)))
    return (u >= np.float32(p)).astype(np.uint8)


def scale_of(p):
    """the kernels' fp32 s = 1.0f / (1.0f - p), as a Python float"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def find_step(seed, block_index, N, p, want, start=0, limit=100000):
    """first step >= start whose mask satisfies want(mask)"""
    for step in range(start, start + limit):
        if want(keep_mask(seed, step, block_index, N, p)):
            return step
    raise RuntimeError("no step found")
