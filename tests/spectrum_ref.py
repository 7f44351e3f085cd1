"""Reference for the trace spectrum (a plain helper, not a conftest).

The definition is restated in numpy integers over the C oracle's edge rows
(oracle.native.span_edges: the row the edge table counts a span in):

  bad(i)  = dur_us[i] > thr_us[row(i)]  or  use_errors and (flags[i] & 1)
  trace t is abnormal (class 1) when any of its spans is bad, else normal
  n_traces[k]       traces of class k (an empty trace is normal)
  svc_traces[k][s]  traces of class k holding >= 1 span of service s
  edge_traces[k][r] the same per edge row
  bad_spans[r]      bad spans of row r

Every result is an integer: GPU results are compared to it bit for bit."""
import numpy as np

import anomod
from oracle import native

U32_MAX = 2**32 - 1
FIELDS = ("n_traces", "svc_traces", "edge_traces", "bad_spans", "trace_abnormal")


def rows_ref(sp, S=None) -> np.ndarray:
    return native.span_edges(sp, S).astype(np.int64)


def spectrum_ref(sp, thr_us=None, use_errors=True, rows=None) -> dict:
    S = len(sp.services)
    E = (S + 2) * S
    nt = sp.n_traces
    rows = rows_ref(sp) if rows is None else rows
    lo, hi = int(sp.trace_ptr[0]), int(sp.trace_ptr[-1])   # the spans that lie in traces
    r = rows[lo:hi]
    svc = sp.svc[lo:hi].astype(np.int64)
    dur = sp.dur_us[lo:hi].astype(np.int64)
    thr = (np.full(E, U32_MAX, np.int64) if thr_us is None
           else np.asarray(thr_us).astype(np.int64))
    assert thr.shape == (E,)
    bad = dur > thr[r]
    if use_errors:
        bad = bad | ((sp.flags[lo:hi] & anomod.FLAG_ERROR) != 0)
    t_of = np.repeat(np.arange(nt, dtype=np.int64), np.diff(sp.trace_ptr).astype(np.int64))
    cls = (np.bincount(t_of, weights=bad, minlength=nt) > 0).astype(np.int64)
    tr = np.unique(t_of * E + r)          # one entry per (trace, row)
    ts = np.unique(t_of * S + svc)        # one entry per (trace, service)
    return {
        "n_traces": np.bincount(cls, minlength=2).astype(np.uint64),
        "svc_traces": np.bincount(cls[ts // S] * S + ts % S,
                                  minlength=2 * S).reshape(2, S).astype(np.uint64),
        "edge_traces": np.bincount(cls[tr // E] * E + tr % E,
                                   minlength=2 * E).reshape(2, E).astype(np.uint64),
        "bad_spans": np.bincount(r[bad], minlength=E).astype(np.uint64),
        "trace_abnormal": cls.astype(np.uint8),
    }


def ochiai_ref(ef, ep, F) -> np.ndarray:
    """ef / sqrt(F * (ef + ep)) in float64, 0 where the denominator is 0."""
    ef = np.asarray(ef).astype(np.float64)
    den = np.sqrt(float(F) * (ef + np.asarray(ep).astype(np.float64)))
    out = np.zeros(ef.shape[0])
    nz = den > 0
    out[nz] = ef[nz] / den[nz]
    return out


def service_ochiai_ref(ref: dict) -> np.ndarray:
    return ochiai_ref(ref["svc_traces"][1], ref["svc_traces"][0], int(ref["n_traces"][1]))


def assert_spectrum_equal(got, ref: dict):
    """got: anomod.TraceSpectrum."""
    for k in FIELDS:
        g = getattr(got, k)
        assert g.dtype == ref[k].dtype and g.shape == ref[k].shape, k
        np.testing.assert_array_equal(g, ref[k], err_msg=k)


def oracle_table(sp) -> anomod.EdgeTable:
    """The C oracle's edge table of sp as an EdgeTable."""
    t = native.finalize(native.edge_aggregate(sp))
    return anomod.EdgeTable(list(sp.services), t["count"], t["errors"], t["sum_us"], t["min_us"],
                            t["max_us"], t["p50_us"], t["p99_us"], t["hist"])


def make_set(S, lens, rng, *, p_root=0.2, p_orphan=0.05, p_error=0.05, dur_hi=1000,
             services=None):
    """Traces of the given lengths over S services: unique ids, a span refers
    to a random earlier span of its trace (or to none / to an id no span
    carries), random services, durations and error flags."""
    lens = np.asarray(lens, np.int64)
    n = int(lens.sum())
    ptr = np.zeros(lens.shape[0] + 1, np.uint64)
    np.cumsum(lens, out=ptr[1:])
    starts = ptr[:-1].astype(np.int64)
    t_of = np.repeat(np.arange(lens.shape[0]), lens)
    pos = np.arange(n) - starts[t_of]
    sid = np.arange(1, n + 1, dtype=np.uint64) + np.uint64(1 << 40)
    pick = starts[t_of] + (rng.random(n) * np.maximum(pos, 1)).astype(np.int64)
    pid = np.where((pos > 0) & (rng.random(n) >= p_root), sid[pick], np.uint64(0))
    orph = (pos > 0) & (rng.random(n) < p_orphan)
    pid[orph] = rng.integers(1, 1 << 39, int(orph.sum()), dtype=np.uint64)
    names = [f"svc{i:03d}" for i in range(S)] if services is None else list(services)
    return anomod.SpanSet(names, ptr, sid.copy(), sid, pid,
                          rng.integers(0, S, n).astype(np.uint16),
                          (rng.random(n) < p_error).astype(np.uint16),
                          rng.integers(0, dur_hi, n).astype(np.uint32))
