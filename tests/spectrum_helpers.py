"""The periodogram rule of ``include/ftk.h`` ("spectrum") restated in numpy float64, and the tolerance the GPU results
are held to against it.  Shared by ``tests/test_wps_spectrum.py`` (CPU) and ``tests/test_gpu_wps_spectrum.py``."""
import numpy as np

U49 = 2.0 ** -49


def taper_weights(N: int, taper: float) -> np.ndarray:
    """Split cosine bell of fraction ``taper``: ``M = floor(taper * N)`` samples at either end, 1 elsewhere."""
    w = np.ones(N, np.float64)
    M = int(np.floor(taper * N))
    if M > 0:
        n = np.arange(M, dtype=np.float64)
        edge = 0.5 * (1.0 - np.cos(np.pi * (2.0 * n + 1.0) / (2.0 * M)))
        w[:M] = edge
        w[N - M:] = edge[::-1]
    return w


def spectrum_ref(v, periods, taper=0.1, detrend=True):
    """``(complex128 [n_per], ssw)`` of ONE run ``v`` (integers): the rule, term by term, the angle from ``n mod p``."""
    v = np.asarray(v, dtype=np.int64)
    N = len(v)
    periods = np.asarray(periods, dtype=np.int64)
    if N == 0:
        return np.zeros(len(periods), np.complex128), 0.0
    m = float(int(v.sum())) / float(N) if detrend else 0.0
    w = taper_weights(N, taper)
    x = (v.astype(np.float64) - m) * w
    n = np.arange(N, dtype=np.int64)
    out = np.zeros(len(periods), np.complex128)
    for k, p in enumerate(periods):
        ang = 2 * np.pi * (n % int(p)).astype(np.float64) / float(p)
        out[k] = complex(np.sum(x * np.cos(ang)), -np.sum(x * np.sin(ang)))
    return out, float(np.sum(w * w))


def spectrum_ref_runs(scores, offsets, periods, taper=0.1, detrend=True):
    """``spectrum_ref`` of every run ``scores[offsets[i]:offsets[i+1]]``: ``(complex128 [n_iv, n_per], ssw [n_iv])``."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n_iv = len(offsets) - 1
    spec = np.zeros((n_iv, len(periods)), np.complex128)
    ssw = np.zeros(n_iv, np.float64)
    for i in range(n_iv):
        spec[i], ssw[i] = spectrum_ref(scores[offsets[i]:offsets[i + 1]], periods, taper, detrend)
    return spec, ssw


def component_tolerance(v, periods) -> np.ndarray:
    """Absolute tolerance per component (re, im) at every period: ``2^-49 * (N + p) * (sum |v| + 1)`` - any summation
    order (``N u sum|x|``), a restarted rotation (``3 p u sum|x|``) and few-ulp differences in the mean, the taper and
    the twiddles, with ``u = 2^-53`` and ``sum|x| <= 2 sum|v|``."""
    v = np.asarray(v, dtype=np.int64)
    total = float(np.abs(v.astype(np.float64)).sum()) + 1.0
    return U49 * (len(v) + np.asarray(periods, dtype=np.float64)) * total


def ssw_tolerance(N: int, ssw: float) -> float:
    """``ssw``: relative ``2^-49 * N``."""
    return U49 * N * abs(ssw)


def assert_spectrum_close(got, got_ssw, v, periods, taper, detrend, what=""):
    """One run's GPU result against the restatement, every component within ``component_tolerance``."""
    want, want_ssw = spectrum_ref(v, periods, taper, detrend)
    tol = component_tolerance(v, periods)
    err_re, err_im = np.abs(got.real - want.real), np.abs(got.imag - want.imag)
    worst = float(np.max(np.maximum(err_re, err_im) / tol)) if len(tol) else 0.0
    assert np.all(err_re <= tol) and np.all(err_im <= tol), (what, len(v), worst)
    assert abs(got_ssw - want_ssw) <= ssw_tolerance(len(v), want_ssw), (what, len(v), got_ssw, want_ssw)
    return worst
