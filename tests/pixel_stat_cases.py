"""Crafted sample streams for the pixel-statistics kernels (tests/test_pixel_stats_host.py on the
CPU, tests/test_gpu_pixel_stats.py on the device; oracle/gen_golden.py takes the reference
fixture's streams from here).

A table is [pixels, budget, 3] float64: row p holds the radiance samples pixel p would trace, in
sample order.  The main table is a 37 x 29 grid (1073 pixels: a multiple of none of 16, 32, 64)
at budget 64; its rows come in families, each aimed at one way the kernels' arithmetic can leave
the reference's (pixel_state.h RecordSample / IsConverged).  Everything is deterministic: fixed
seeds, and the near-threshold amplitudes found by bisection in the CPU oracle.
"""
import functools

import numpy as np

import oracle_ctypes as orc

WIDTH, HEIGHT = 37, 29
NPIX = WIDTH * HEIGHT
BUDGET = 64
REL0 = float(np.float32(0.05))  # wavefront.cc kRelThresh (a float), the shipped default
MIN0 = 16
TINY = 2.0 ** -900  # div_by_count takes the division below this |delta|

# (rel, min_spp): the shipped default first
PAIRS = [(REL0, MIN0), (0.02, 4), (1e-3, 1), (0.0, MIN0), (1e-200, MIN0), (1.0, MIN0), (1e6, MIN0),
         (float("inf"), MIN0), (-0.05, MIN0), (REL0, 0), (REL0, BUDGET + 1)]


def ulps(x, k):
    """The double k ulps from x > 0 (k may be negative)."""
    return float((np.array([x], np.float64).view(np.int64) + k).view(np.float64)[0])


def two_valued(mean, a, budget=BUDGET):
    """mean + a, mean - a, mean + a, ... in all three channels."""
    s = np.where(np.arange(budget) % 2 == 0, mean + a, mean - a)
    return np.repeat(s[:, None], 3, axis=1)


def decision(mean, a, n, rel):
    """IsConverged after exactly n samples of two_valued(mean, a), in the oracle."""
    r = orc.pixel_replay("adaptive", two_valued(mean, a, n)[None], n, rel)
    return bool(r["conv"][0])


def flip_amplitude(mean, n, rel):
    """The largest amplitude a (found by bisection over the doubles) with the pixel converged at
    sample n while the next double is not: the decision flips between two adjacent doubles."""
    lo, hi = abs(mean) * 1e-9 + 1e-12, 10.0 * max(abs(mean), 1e-3) * max(rel, 1e-6) * np.sqrt(n) + 1.0
    assert decision(mean, lo, n, rel) and not decision(mean, hi, n, rel)
    ilo, ihi = (int(np.array([v], np.float64).view(np.int64)[0]) for v in (lo, hi))
    while ihi - ilo > 1:
        mid = (ilo + ihi) // 2
        if decision(mean, float(np.array([mid], np.int64).view(np.float64)[0]), n, rel):
            ilo = mid
        else:
            ihi = mid
    return float(np.array([ilo], np.int64).view(np.float64)[0])


# near-threshold rows: (rel, n, mean) with n >= the pair's min_spp
NEAR = [(REL0, 16, 0.5), (REL0, 17, 1.0), (REL0, 24, 3.0), (REL0, 33, 0.5), (REL0, 48, 1.0), (REL0, 63, 0.25),
        (REL0, 64, 2.0), (REL0, 40, -1.5), (0.02, 4, 1.0), (0.02, 5, 0.5), (0.02, 40, 2.0), (1.0, 16, 1.0),
        (1.0, 31, 0.5)]


def _families():
    """[(family name, rows [n, BUDGET, 3], per-row notes)] of the main table, before shuffling."""
    rng = np.random.default_rng(20240607)
    fam = []

    def add(name, rows, notes=None):
        rows = np.asarray(rows, np.float64)
        assert rows.shape[1:] == (BUDGET, 3), (name, rows.shape)
        fam.append((name, rows, notes if notes is not None else [None] * len(rows)))

    # constant rows: m2 == 0 exactly
    consts = [0.0, -0.0, 1.0, -1.0, 0.5, 1e-4, -1e-4, 5e-4, 1e-3, -1e-3, 9.999e-4, 1e-300, -3.7, 1e10, 0.1, 1e-320,
              1e154, -1e200, 1.7976931348623157e308, 2.0 ** -900, 3.0, 1e-3 + 1e-19, 0.7, 123.456]
    rows = [np.full((BUDGET, 3), c) for c in consts]
    rows += [np.tile(np.array([0.0, -0.0, 2.5]), (BUDGET, 1)), np.tile(np.array([1e-4, 1.0, -1e10]), (BUDGET, 1))]
    add("constant", rows)

    # near-threshold rows: the amplitude at which the decision at sample n flips, moved -4 .. +4 ulps
    rows, notes = [], []
    for rel, n, mean in NEAR:
        a = flip_amplitude(mean, n, rel)
        for k in range(-4, 5):
            rows.append(two_valued(mean, ulps(a, k)))
            notes.append((rel, n, mean, ulps(a, k)))
    add("near_threshold", rows, notes)

    # clamp rows: |mean| straddling 1e-3, the amplitude near the threshold of the clamped form
    rows = []
    for m in [ulps(1e-3, -1), 1e-3, ulps(1e-3, 1), 0.9e-3, 1.1e-3, 0.0, -ulps(1e-3, -1), -1e-3, -ulps(1e-3, 1), -0.9e-3]:
        for f in (0.97, 1.0, 1.03):
            rows.append(two_valued(m, f * REL0 * 1e-3 * np.sqrt(19.0)))  # the flip at n = 20 when |mean| <= 1e-3
    add("clamp", rows)

    # one noisy channel, the other two constant: the conjunction over the channels
    rows = []
    for ch in range(3):
        for sd in (0.01, 0.05, 0.1, 0.2, 0.3, 0.5, 0.8, 1.0, 2.0, 5.0):
            r = np.tile(np.array([0.4, 1.0, 2.5]), (BUDGET, 1))
            r[:, ch] += sd * r[0, ch] * rng.standard_normal(BUDGET)
            rows.append(r)
    add("one_noisy_channel", rows)

    # magnitudes: mu * mu and m2 overflow; tiny values and deltas below, at and above 2^-900
    rows = []
    for base in (1e150, 1e160, 1e200, 1e250, 1e300, 1e307):
        for noise in (1e-3, 0.3):
            rows.append(base * (1.0 + noise * rng.standard_normal((BUDGET, 3))))
    for base in (1e-160, 1e-250, TINY * 8, TINY, TINY / 8, 1e-300, 1e-310, 5e-324 * 1000):
        for noise in (1e-3, 0.5):
            rows.append(base * (1.0 + noise * rng.standard_normal((BUDGET, 3))))
    for first in (TINY, ulps(TINY, -1), ulps(TINY, 1), -TINY, -ulps(TINY, -1)):
        r = np.zeros((BUDGET, 3))  # sample 1's delta is `first` exactly; later deltas are multiples near it
        r[0] = first
        r[1:] = first * rng.integers(-3, 4, (BUDGET - 1, 3))
        rows.append(r)
    add("magnitudes", rows)

    # non-finite rows: one inf, -inf or NaN at sample 1, at min_spp and after it
    rows = []
    for bad in (np.inf, -np.inf, np.nan):
        for at in (0, MIN0 - 1, 20):
            for ch in range(3):
                r = 0.5 + 0.3 * rng.standard_normal((BUDGET, 3))
                r[at, ch] = bad
                rows.append(r)
    add("non_finite", rows)

    # cancellation rows: 1e16-sized values that cancel, interleaved with ones of order 1
    rows = []
    for i in range(40):
        r = np.zeros((BUDGET, 3))
        for ch in range(3):
            big = rng.choice([1e16, 3e16, 1e17, 2.5e15], BUDGET // 4 + 1) * rng.choice([-1.0, 1.0], BUDGET // 4 + 1)
            s = []
            for b in big:
                s += [b, rng.uniform(0.1, 2.0), -b, rng.uniform(0.1, 2.0)]
            r[:, ch] = np.array(s[:BUDGET])
        rows.append(r)
    add("cancellation", rows)

    # heavy-tailed rows: log-normal fireflies, which run to the budget
    add("heavy_tailed", np.exp(-1.0 + 2.5 * rng.standard_normal((40, BUDGET, 3))))

    # rows that stop at exactly min_spp, at budget - 1 and at budget (under the default pair)
    rows, notes = [], []
    for n in (MIN0, BUDGET - 1, BUDGET):
        for mean in (0.5, 1.0, 4.0, -2.0):
            a = 1e-3 * abs(mean) if n == MIN0 else flip_amplitude(mean, n, REL0) * (1.0 - 1e-6)
            rows.append(two_valued(mean, a))
            notes.append(n)
    add("stops_at", rows, notes)

    # the rest: noisy rows whose convergence points spread from min_spp to beyond the budget
    n_rest = NPIX - sum(len(r) for _, r, _ in fam)
    assert n_rest > 200
    mean = rng.uniform(0.05, 3.0, (n_rest, 1, 3))
    sd = mean * np.exp(rng.uniform(np.log(0.02), np.log(0.6), (n_rest, 1, 1)))
    add("noisy", mean + sd * rng.standard_normal((n_rest, BUDGET, 3)))
    return fam


@functools.lru_cache(maxsize=None)
def main_table():
    """(table [NPIX, BUDGET, 3], family [NPIX] (index into names), names, notes [NPIX]): the
    families' rows shuffled over the grid, so that k_adapt_plan's 3 x 3 neighbourhoods mix them."""
    fam = _families()
    rows = np.concatenate([r for _, r, _ in fam])
    family = np.concatenate([np.full(len(r), i) for i, (_, r, _) in enumerate(fam)])
    notes = [n for _, _, ns in fam for n in ns]
    assert len(rows) == NPIX
    perm = np.random.default_rng(7).permutation(NPIX)
    table = np.ascontiguousarray(rows[perm])
    table.setflags(write=False)
    return table, family[perm], [f[0] for f in fam], [notes[i] for i in perm]


def rows_of(name):
    table, family, names, _ = main_table()
    return np.flatnonzero(family == names.index(name))


def fixture_streams():
    """The streams of tests/golden/pixelstate_edges.npz (the reference's own RecordSample /
    IsConverged on them, oracle/gen_golden.py): two rows of every family cut to 20 samples, and
    the near-threshold rows whose flip is at n <= 24 with the amplitude moved -1, 0, +1 ulps, cut
    just after the flip.  A few hundred samples."""
    table, family, names, notes = main_table()
    out = []
    for name in names:
        if name != "near_threshold":
            out += [table[p, :20] for p in rows_of(name)[:2]]
    for rel, n, mean in NEAR:
        if n <= 24:
            a = flip_amplitude(mean, n, rel)
            out += [two_valued(mean, ulps(a, k), n + 1) for k in (-1, 0, 1)]
    return out


def pack_streams(streams):
    """ref_harness pixelstate's input: (n, then n samples of 3 doubles) per stream."""
    return np.ascontiguousarray(np.concatenate([np.concatenate([[len(s)], np.ravel(s)]) for s in streams]))


def unpack_streams(seq):
    out, k = [], 0
    while k < len(seq):
        n = int(seq[k])
        out.append(seq[k + 1:k + 1 + 3 * n].reshape(n, 3))
        k += 1 + 3 * n
    return out


BUDGET_LONG = 200


@functools.lru_cache(maxsize=None)
def long_table():
    """[NPIX, 200, 3]: noisy rows that converge anywhere from min_spp 16 to beyond 200 samples, and
    the main table's rows continued periodically (several phases, batches of every size)."""
    rng = np.random.default_rng(99)
    mean = rng.uniform(0.05, 3.0, (NPIX, 1, 3))
    sd = mean * np.exp(rng.uniform(np.log(0.02), np.log(1.2), (NPIX, 1, 1)))
    t = mean + sd * rng.standard_normal((NPIX, BUDGET_LONG, 3))
    main = main_table()[0]
    take = np.arange(0, NPIX, 3)
    t[take] = np.concatenate([main[take]] * 4, axis=1)[:, :BUDGET_LONG]
    t = np.ascontiguousarray(t)
    t.setflags(write=False)
    return t


# The megakernel's AdaptiveSampler(min, max, threshold): tables of max + 1 samples
MK_MAX = 24
MK_SETTINGS = [(5, 0.05), (7, 0.02), (1, 0.5)]  # (min_samples, threshold) at max_samples MK_MAX


@functools.lru_cache(maxsize=None)
def mk_table():
    """[rows, MK_MAX + 1, 3].  A first sample c followed by zeros keeps the running sum `pixel` at
    c, so sum_sq / n - mean * mean is 0 up to rounding: where it rounds below zero the error is NaN
    and the pixel goes on, where it does not the pixel stops at min.  (1 / n is exact at n = 8,
    where these rows stop at the latest: hence the odd min_samples.)  Zeros stop at min; noisy
    rows stop in between or run to max + 1; the main table's rows bring the non-finite values and
    the huge ones, whose inf - inf never stops."""
    rng = np.random.default_rng(5)
    k = MK_MAX + 1
    rows = []
    for c in np.concatenate([rng.uniform(0.01, 3.0, 120), [0.1, 0.3, 0.7, 1.1, 1e-3, 1e8]]):
        r = np.zeros((k, 3))
        r[0] = c * np.array([1.0, 0.9, 1.3])
        rows.append(r)
    rows.append(np.zeros((k, 3)))
    rows.append(np.full((k, 3), -0.0))
    for sd in np.exp(rng.uniform(np.log(0.01), np.log(2.0), 120)):
        rows.append(rng.uniform(0.1, 2.0, 3) * (1.0 + sd * rng.standard_normal((k, 3))))
    t = np.concatenate([np.array(rows), main_table()[0][::4, :k]])
    t = np.ascontiguousarray(t)
    t.setflags(write=False)
    return t


def bits(a):
    """The array's bytes as unsigned integers: equal bits, NaN payloads and zero signs included."""
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])
