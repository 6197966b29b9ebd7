"""A numpy model of agpt_render_adaptive's contract (include/agpt.h): rounds run one after another in float32 on per-sample
radiance.  Pixels are the elements of the buffer as given (any layout: the decision is per pixel)."""
import numpy as np

F = np.float32


def luminance(rgb):
    """agpt_math.h's luminance, rounded op by op like the device code (-ffp-contract=off)."""
    rgb = np.asarray(rgb, F)
    return (F(0.212671) * rgb[..., 0] + F(0.715160) * rgb[..., 1]) + F(0.072169) * rgb[..., 2]


def reject(clr):
    """The NaN / inf reject of myapp.cpp:169-172 (k_accumulate): such a sample adds zero."""
    clr = np.asarray(clr, F)
    with np.errstate(invalid="ignore", over="ignore"):
        bad = np.isnan(clr).any(-1) | np.isinf(luminance(clr))
    return np.where(bad[..., None], F(0), clr), bad


def test_value(S, M, n, rel_error, abs_floor):
    """(lhs, rhs) of the stop test sqrt(var / n) <= rel_error * max(mu, abs_floor), in float32, for n >= 2.  Every max is fmaxf
    (include/agpt.h): a NaN operand yields the other one, so a NaN moment2 is a variance of 0."""
    nf = np.asarray(n, F)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        mu = luminance(S) / nf
        var = np.fmax(F(0), np.asarray(M, F) / nf - mu * mu) * nf / (nf - F(1))
        lhs = np.sqrt(var / nf)
        rhs = F(rel_error) * np.fmax(mu, F(abs_floor))
    return lhs, rhs


def decide(S, M, n, min_spp, max_spp, rel_error, abs_floor, near_rel=1e-4):
    """-> (active, near): active pixels of a round; near marks test values within rel near_rel of the threshold."""
    tested = (n >= min_spp) & (n < max_spp)
    active = n < max_spp
    near = np.zeros(n.shape, bool)
    if rel_error > 0:
        lhs, rhs = test_value(S, M, np.maximum(n, 2), rel_error, abs_floor)
        stop = lhs <= rhs
        active &= (n < min_spp) | ~stop
        with np.errstate(invalid="ignore"):   # (inf - inf where both sides are infinite: not near)
            near = tested & (np.abs(lhs.astype(np.float64) - rhs) <= near_rel * np.abs(rhs.astype(np.float64)))
    return active, near


def run(samples, min_spp, max_spp, step_spp, rel_error, abs_floor=0.0, counts=None, accum=None, moment2=None):
    """samples[n_samples, ...pixels, 3]: the radiance of sample s of every pixel (n_samples >= max_spp).  Starts from counts /
    accum[..., 3] / moment2 (zeros: a fresh frame) and runs rounds until no pixel is active.
    -> dict(counts, accum (rgb), moment2, near (a decision within rel 1e-4 of the threshold), rounds, outliers)."""
    samples = np.asarray(samples, F)
    shape = samples.shape[1:-1]
    n = np.zeros(shape, np.int64) if counts is None else np.array(counts, np.int64)
    S = np.zeros(shape + (3,), F) if accum is None else np.array(accum, F)[..., :3].copy()
    M = np.zeros(shape, F) if moment2 is None else np.array(moment2, F)
    near = np.zeros(shape, bool)
    rounds = outliers = 0
    while True:
        act, nr = decide(S, M, n, min_spp, max_spp, rel_error, abs_floor)
        near |= nr
        if not act.any():
            break
        idx = np.nonzero(act)
        for k in range(step_spp):
            clr, bad = reject(samples[(n[idx] + k,) + idx])
            outliers += int(bad.sum())
            S[idx] = S[idx] + clr
            Y = luminance(clr)
            M[idx] = M[idx] + Y * Y
        n[idx] += step_spp
        rounds += 1
    return dict(counts=n, accum=S, moment2=M, near=near, rounds=rounds, outliers=outliers)
