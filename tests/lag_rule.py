"""The detector lag correction in numpy (test infrastructure), written from the statement in
include/paris_hip.h and not from the library's code: the coefficients, the fp32 pixel rule with the exact fused multiply-add of
tests/beam_hardening_rule.py, and the float64 forward model and inverse the physics tests use. Plus wrong restatements that a test
must tell from the right one, and the models and inputs the tests share. A helper, not a test."""
import numpy as np

from beam_hardening_rule import bits, fmaf, same_pixels  # noqa: F401  (same_pixels and bits are used by the tests)

# the four-term model of DESIGN.md section 4.20, (b_n, a_n) per term, and its truncations: b_0 = 0.9503 with all four
TERMS4 = ((7.1e-6, 2.5e-3), (1.1e-4, 2.1e-2), (1.7e-3, 1.6e-1), (1.9e-2, 1.0))
MODELS = {n: TERMS4[:n] for n in (1, 2, 3, 4)}
STARTS = ("steady", "rest")
FULL_SCALE = 60000.0
NAN_PAYLOAD = 0x7FC12345


def coefficients64(terms):
    """(g, c, w, inv_b, b0) in float64 from the model's float32 parameters"""
    b = np.array([np.float32(t[0]) for t in terms], np.float64)
    a = np.array([np.float32(t[1]) for t in terms], np.float64)
    g = np.exp(-a)
    b0 = 1.0 - float(sum(bn / (1.0 - gn) for bn, gn in zip(b, g)))      # ascending n
    big_b = b0
    for bn in b:
        big_b = big_b + bn
    return g, b * g / big_b, 1.0 / (1.0 - g), 1.0 / big_b, b0


def coefficients(terms):
    """the same, each rounded once to float32 (b0 stays a float64)"""
    g, c, w, inv_b, b0 = coefficients64(terms)
    return g.astype(np.float32), c.astype(np.float32), w.astype(np.float32), np.float32(inv_b), b0


def correct(terms, frames, dark=None, start="steady", state=None, started=False, wrong=None):
    """The rule on frames[f], f in time order. Returns (corrected, state, started) like paris_amd.backend.lag_correct_host.
    wrong: one of WRONG -- a restatement that is NOT the rule."""
    g, c, w, inv_b, _ = coefficients(terms)
    n_terms = len(terms)
    out = np.array(frames, np.float32)
    shape = out.shape[1:]
    d = np.zeros(shape, np.float32) if dark is None else np.asarray(dark, np.float32).reshape(shape)
    s = np.zeros((n_terms,) + shape, np.float32) if state is None else np.array(state, np.float32)
    started = bool(started) and state is not None
    order = range(n_terms - 1, -1, -1) if wrong == "terms summed in reverse order" else range(n_terms)
    with np.errstate(all="ignore"):
        for f in range(out.shape[0]):
            i = out[f]
            y = (i - d).astype(np.float32)
            finite = np.isfinite(y)
            if not started or wrong == "steady applied to every frame":
                for n in range(n_terms):
                    s[n] = np.where(finite, (w[n] * y).astype(np.float32), np.float32(0)) if start == "steady" else np.float32(0)
            if wrong == "state updated before x is formed":
                for n in range(n_terms):
                    s[n] = fmaf(g[n], s[n], (y * inv_b).astype(np.float32))
            acc = (y * inv_b).astype(np.float32)
            for n in order:
                if wrong == "multiply-then-add instead of fmaf":
                    acc = (acc + ((-c[n]) * s[n]).astype(np.float32)).astype(np.float32)
                else:
                    acc = fmaf(-c[n], s[n], acc)
            x = np.where(finite, acc, np.float32(0)).astype(np.float32)
            back = x if wrong == "dark not added back" else (x + d).astype(np.float32)
            out[f] = np.where(finite, back, i)
            if wrong != "state updated before x is formed":
                for n in range(n_terms):
                    s[n] = fmaf(g[n], s[n], x)
            started = True
    return out, s, started


WRONG = ("state updated before x is formed", "terms summed in reverse order", "multiply-then-add instead of fmaf",
         "steady applied to every frame", "dark not added back")


# ---- float64: the detector's forward model and its exact inverse ------------------------------------------------------------------

def forward64(terms, x, start="steady"):
    """y_k = B x_k + sum_n b_n g_n S_n,k with S_n,(k+1) = x_k + g_n S_n,k; steady: the first view had been seen for ever"""
    g, _, w, inv_b, _ = coefficients64(terms)
    b = np.array([np.float32(t[0]) for t in terms], np.float64)
    x = np.asarray(x, np.float64)
    s = [w[n] * x[0] if start == "steady" else np.zeros_like(x[0]) for n in range(len(terms))]
    y = np.empty_like(x)
    for k in range(x.shape[0]):
        acc = x[k] / inv_b
        for n in range(len(terms)):
            acc = acc + b[n] * g[n] * s[n]
        y[k] = acc
        for n in range(len(terms)):
            s[n] = x[k] + g[n] * s[n]
    return y


def inverse64(terms, y, start="steady"):
    """the rule in float64 with float64 coefficients, finite pixels only"""
    g, c, w, inv_b, _ = coefficients64(terms)
    y = np.asarray(y, np.float64)
    s = [w[n] * y[0] if start == "steady" else np.zeros_like(y[0]) for n in range(len(terms))]
    x = np.empty_like(y)
    for k in range(y.shape[0]):
        acc = y[k] * inv_b
        for n in range(len(terms)):
            acc = acc - c[n] * s[n]
        x[k] = acc
        for n in range(len(terms)):
            s[n] = acc + g[n] * s[n]
    return x


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

def special_frames(shape, seed=0):
    """counts between 3000 and 60000 with the values the rule has clauses or roundings for sprinkled in: negative, denormal, +-0,
    a NaN with a payload and both infinities"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(3000.0, FULL_SCALE, shape).astype(np.float32)
    flat = f.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, 1.1754944e-38, -250.5, -1.0],
                       np.float32)
    for rep in range(max(1, flat.size // 400)):
        at = rng.choice(flat.size, special.size, replace=False)
        flat[at] = special
        flat.view(np.uint32)[at[0]] = NAN_PAYLOAD
    return f


def dark_frame(shape, seed=0):
    """a dark of about 1000 counts with a dead pixel's worth of oddities: one NaN, one 0"""
    rng = np.random.default_rng(1000 + seed)
    d = rng.uniform(900.0, 1100.0, shape).astype(np.float32)
    d.reshape(-1)[[1, d.size // 2]] = [np.nan, 0.0]
    return d


def edge_sweep(n_pixels=64, n_frames=400, seed=5):
    """float64 counts: pixel p sees 60000 until the edge passes it at frame 40 + 5 p, then 3000; with noise of sqrt(counts)"""
    rng = np.random.default_rng(seed)
    k = np.arange(n_frames)[:, None]
    clean = np.where(k < 40 + 5 * np.arange(n_pixels)[None, :], FULL_SCALE, 3000.0)
    return clean + rng.standard_normal(clean.shape) * np.sqrt(clean)


def constant_with_noise(n_pixels=16, n_frames=4000, seed=6):
    rng = np.random.default_rng(seed)
    clean = np.full((n_frames, n_pixels), 30000.0)
    return clean + rng.standard_normal(clean.shape) * np.sqrt(clean)
