"""Shared by tests/test_guard_kernels_gpu.py and tests/test_guard_step_gpu.py: the launch geometry of atomnas_grad_guard (csrc/optim.hip
k_grad_sumsq / k_guard_verdict) and the error bound of its norm that follows from it.

Geometry: 256 threads per workgroup; a thread loads UNROLL 16-byte pieces per sweep, so a workgroup covers SWEEP = 256 * UNROLL pieces
per sweep and the grid min(ceil(pieces / SWEEP), MAX_BLOCKS) workgroups; one sweep of the capped grid is MAX_BLOCKS * SWEEP * 4 floats.

Bound (derived from the summation order, not from a run).  Every term of the sum is a square, so all partial sums are non-negative
and the relative error of the fp32 sum is at most (number of roundings on the longest path of a value) * 2^-24 to first order.  That
path is:
    1                     the square itself
    2                     (x0^2 + x1^2) + (x2^2 + x3^2) inside a 16-byte piece
    sweeps                one addition to the thread's accumulator per sweep of the grid
    2                     (a0 + a1) + (a2 + a3), the four accumulators of a thread
    1                     the ragged tail of up to 3 floats (thread 0..2 of workgroup 0)
    6                     xor-shuffle levels of a 64-lane wave
    3                     ((w0 + w1) + w2) + w3, the four waves of a workgroup
    ceil(blocks / 256)    stage 2: thread t adds partials t, t + 256, ...
    8                     stage 2: the 256-leaf tree
The norm is sqrt(sum) * scale: the square root halves the relative error of the sum and adds one rounding, the scale another.  The
bound used is TWICE chain * 2^-24, relative to the float64 norm, which covers chain / 2 + 2 roundings for every chain >= 2.
For n = one sweep of the capped grid + 3 the chain is 28: 3.3e-6."""

UNROLL = 4
SWEEP = 256 * UNROLL        # 16-byte pieces per workgroup and sweep
MAX_BLOCKS = 1024           # == atomnas_grad_guard_ws_floats()
ONE_SWEEP_FLOATS = MAX_BLOCKS * SWEEP * 4   # 4,194,304 floats, 16 MiB

GUARD_OK, GUARD_SCALE, GUARD_NORM, GUARD_COEF, GUARD_SKIPPED, GUARD_CLIPPED = range(6)


def geometry(n):
    """-> (workgroups, sweeps) of the stage-1 launch over n floats"""
    n4 = n // 4
    blocks = min(max((n4 + SWEEP - 1) // SWEEP, 1), MAX_BLOCKS)
    sweeps = (n4 + blocks * SWEEP - 1) // (blocks * SWEEP)
    return blocks, sweeps


def chain(n):
    blocks, sweeps = geometry(n)
    return 1 + 2 + sweeps + 2 + 1 + 6 + 3 + (blocks + 255) // 256 + 8


def norm_rel_bound(n):
    return 2.0 * chain(n) * 2.0 ** -24
