"""The clipped momentum-SGD step of include/detectorch_optim_hip.h restated in numpy: float32 with one rounding per operation in
the header's order (step32), the same step in float64 as the yardstick (step64), the float64 norm, and the chunk table of
dtc_sgd_plan.  Test infrastructure only."""
import numpy as np

f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
CHUNK, BODY_CHUNKS = 4096, 2048


def norm64(grads):
    """sqrt(sum g^2) over a list of arrays in float64: the squares are exact, numpy's pairwise sum per array and math.fsum over the
    arrays leave a relative error of a few 1e-16, nothing next to a float32 ulp"""
    import math
    with np.errstate(all="ignore"):
        return math.sqrt(math.fsum(float(np.sum(np.square(np.asarray(g, np.float64)))) for g in grads))


def coef32(total_norm, max_norm):
    """min(1, max_norm / (total_norm + 1e-6f)) in float32, a NaN quotient kept"""
    with np.errstate(all="ignore"):
        q = f32(max_norm) / (f32(total_norm) + f32(1e-6))
    return q if not q > f32(1) else f32(1)


def step32(params, grads, bufs, coef, hyper, groups, momentum):
    """One step in place on lists of float32 arrays: gc = g * coef; d = gc + wd * p; buf = momentum * buf + d; p = p - lr * buf,
    every operation rounded to float32.  hyper: [(lr, wd)] per group."""
    coef, m = f32(coef), f32(momentum)
    with np.errstate(all="ignore"):
        for p, g, b, k in zip(params, grads, bufs, groups):
            assert p.dtype == g.dtype == b.dtype == np.float32
            lr, wd = f32(hyper[k][0]), f32(hyper[k][1])
            gc = g * coef
            d = gc + wd * p
            b[...] = m * b + d
            p[...] = p - lr * b


def step64(params, grads, bufs, hyper, groups, momentum, max_norm):
    """The same step in float64 on float64 arrays, the norm and the clip factor included (eps 1e-6 as torch).  -> (norm, coef)"""
    total = float(np.sqrt(sum(float(np.sum(np.square(g))) for g in grads)))
    coef = min(1.0, max_norm / (total + 1e-6))
    for p, g, b, k in zip(params, grads, bufs, groups):
        lr, wd = hyper[k]
        b[...] = momentum * b + (g * coef + wd * p)
        p[...] = p - lr * b
    return total, coef


def chunk_elems(total):
    chunk = CHUNK
    while -(-total // chunk) > BODY_CHUNKS:
        chunk <<= 1
    return chunk


def chunk_table(counts):
    """[(tensor, offset, count)] as dtc_sgd_plan lays the chunks out"""
    chunk = chunk_elems(sum(counts))
    return [(i, off, min(chunk, n - off)) for i, n in enumerate(counts) for off in range(0, n, chunk)]
