"""CLI:  python -m anomod features <trace file|dir> [--metrics PATH] [--out FILE]
                                 [--spectrum] [--critical-path] [--shapes]
                                 [--error-origins] [--repeats] [--transit]
                                 [--trace-step S [--trace-load]]
                                 [--exemplars K]
                                 [--trace-step S --symptom-corr [--walk correlation]]
                                 [--baseline <trace file|dir>]
       python -m anomod jaeger-to-csv <all_traces.json> <all_traces.csv>

Computes the RCA features of one experiment on the GPU and writes them as JSON:
the call-graph edge table (count, errors, mean/min/max, p50/p99 per edge), the
per-service anomaly scores and the PageRank root-cause ranking.  It slots in
where the reference's bash orchestration calls its converters
(collect_trace.sh:70 ``python jaeger_to_csv.py ...``;
collect_all_modalities.sh:238 ``python3 trace_collector.py ...``).
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

from . import features, load_experiment, rank


def shapes_doc(census, spans, base=None, top: int = 20) -> dict:
    """The "shapes" object of the features JSON: distinct count, off-tree
    spans and the top shapes (hex fingerprint, count, abnormal, exemplar trace
    with its span count and services, and `new` against the baseline census:
    None without one)."""
    k = min(top, int(census.shape.shape[0]))
    new = census.novel(base)[:k].tolist() if base is not None else [None] * k
    holds = census.service_sets(spans)[:k]
    ptr = spans.trace_ptr
    rows = []
    for i in range(k):
        t = int(census.first_trace[i])
        rows.append({"shape": f"{int(census.shape[i]):016x}", "count": int(census.count[i]),
                     "abnormal": int(census.abnormal[i]), "exemplar_trace": t,
                     "exemplar_spans": int(ptr[t + 1]) - int(ptr[t]),
                     "services": [s for s, h in zip(census.services, holds[i]) if h],
                     "new": new[i]})
    return {"distinct": int(census.n_shapes), "off_tree_spans": int(census.off_tree_spans),
            "top": rows}


def error_origins_doc(eo) -> dict:
    """The "error_origins" object of the features JSON: per service the
    failures that started in it (origin), the error spans that relayed a
    callee's failure (propagated), the origins that reached their trace's
    entry (surfaced) and the mean hops of the origins; error_spans and
    loop_spans of the whole set."""
    org, prop = eo.per_service("origin"), eo.per_service("propagated")
    surf, hops = eo.per_service("surfaced"), eo.mean_hops()
    return {"error_spans": int(eo.error_spans), "loop_spans": int(eo.loop_spans),
            "services": {s: {"origin": int(org[i]), "propagated": int(prop[i]),
                             "surfaced": int(surf[i]), "mean_hops": float(hops[i])}
                         for i, s in enumerate(eo.services)}}


def call_repeats_doc(rep) -> dict:
    """The "call_repeats" object of the features JSON: per callee service the
    logical calls (groups), the calls beyond the first of a group (repeats),
    the groups that repeated around a failure (retried = recovered +
    exhausted), the members that started after a failure of their group had
    ended (after_error; 0 without start times: `timed`) and the largest
    group."""
    cols = {k: rep.per_service(k) for k in ("groups", "repeats", "retried", "recovered",
                                            "exhausted", "after_error", "size_max")}
    return {"timed": bool(rep.timed), "grouped_spans": int(rep.grouped_spans),
            "max_size": int(rep.max_size),
            "services": {s: {k: int(v[i]) for k, v in cols.items()}
                         for i, s in enumerate(rep.services)}}


def call_transit_doc(tr) -> dict:
    """The "call_transit" object of the features JSON: the calls, the paired
    ones among them and, per callee service over the cross-service incoming
    rows, the paired calls, the request / response records with their mean
    gap in microseconds (None without a record) and the largest row p99 of
    each table (None without one), and the early (clock skew), late
    (abandoned) and untimed calls."""
    S = len(tr.services)
    cols = {k: tr.per_service(k) for k in ("paired", "early", "late", "untimed")}

    def table(t, name):
        cnt, tot = tr.per_service(name + ".count"), tr.per_service(name + ".sum_us")
        p99 = np.where(t.count[:S * S] > 0, np.nan_to_num(t.p99_us[:S * S], nan=-1.0), -1.0)
        p99 = p99.reshape(S, S).copy()
        np.fill_diagonal(p99, -1.0)
        top = p99.max(axis=0)
        return [{"records": int(cnt[i]),
                 "mean_us": float(tot[i]) / float(cnt[i]) if cnt[i] else None,
                 "p99_us": float(top[i]) if top[i] >= 0 else None} for i in range(S)]

    req, resp = table(tr.request, "request"), table(tr.response, "response")
    return {"calls": int(tr.calls), "paired": int(tr.paired),
            "services": {s: {"paired": int(cols["paired"][i]), "request": req[i],
                             "response": resp[i], "early": int(cols["early"][i]),
                             "late": int(cols["late"][i]), "untimed": int(cols["untimed"][i])}
                         for i, s in enumerate(tr.services)}}


def edge_load_doc(load) -> dict:
    """The "edge_load" object of the features JSON: the window range, the
    spans that touch no window and, per active edge, the busy time and the
    carried calls of every window."""
    S = len(load.services)
    rows = []
    for r in load.active_rows().tolist():
        p, c = divmod(r, S)
        rows.append({"parent": "ROOT" if p == S else "ORPHAN" if p == S + 1 else load.services[p],
                     "child": load.services[c],
                     "busy_us": [int(v) for v in load.busy_us[:, r]],
                     "carried": [int(v) for v in load.carried[:, r]]})
    return {"t0_us": int(load.t0_us), "step_us": int(load.step_us),
            "windows": int(load.n_windows), "outside": int(load.outside), "edges": rows}


def _key_doc(key) -> dict:
    labels = key[1] if len(key) > 1 else ()
    return {"name": str(key[0]), "labels": {str(k): str(v) for k, v in labels}}


def symptom_correlates_doc(sc, top: int = 10) -> list[dict]:
    """The "symptom_correlates" list of the features JSON: the `top` trace
    columns and metric series that move most with the front-door latency:
    {kind ("trace" | "metric"), name, labels, r, n (common windows)}."""
    return [{"kind": row["kind"], **_key_doc(row["key"]), "r": row["r"], "n": row["n"]}
            for row in sc.top(top)]


def _exemplar_calls(ex, spans, row: int, names: dict) -> list[dict]:
    ids = [names.get(t, t) for t in ex.trace_ids(spans, row)]
    return [{"trace_id": ids[j], "span_id": f"{int(ex.span_id[row, j]):016x}",
             "dur_us": int(ex.dur_us[row, j]), "error": bool(int(ex.flags[row, j]) & 1),
             "start_us": int(ex.start_us[row, j])} for j in range(len(ids))]


def exemplars_doc(feats, spans, ranking, top: int = 5, trace_file=None) -> dict:
    """The "exemplars" object of the features JSON: for each of the `top`
    ranked services, "slow" — its incoming edge with the largest p99_us and
    that edge's slowest calls — and "errors" — its incoming edge with the most
    errors and that edge's slowest failed calls (None when no incoming edge
    holds a span / an error).  A call is {trace_id, span_id (hex), dur_us,
    error, start_us}, slowest first.  trace_id is the set's own id
    (EdgeExemplars.trace_ids); for a set decoded without id strings it is
    looked up in `trace_file` by its hash, and stays the hash in hex when the
    file does not hold it."""
    edges, ex, err_ex = feats.edges, feats.exemplars, feats.error_exemplars
    S = edges.n_services
    out = {}
    picked = []
    for name, _ in ranking[:top]:
        c = edges.services.index(name)
        rows = np.arange(S + 2) * S + c
        entry = {"slow": None, "errors": None}
        p99 = np.where(edges.count[rows] > 0, np.nan_to_num(edges.p99_us[rows], nan=-1.0), -1.0)
        if (p99 >= 0).any():
            r = int(rows[int(np.argmax(p99))])
            entry["slow"] = {"parent": edges.parent_name(r // S), "child": name,
                             "p99_us": float(edges.p99_us[r]),
                             "calls": (ex, r)}
        if edges.errors[rows].any():
            r = int(rows[int(np.argmax(edges.errors[rows]))])
            entry["errors"] = {"parent": edges.parent_name(r // S), "child": name,
                               "errors": int(edges.errors[r]),
                               "calls": (err_ex, r)}
        out[name] = entry
        picked += [e["calls"] for e in entry.values() if e is not None]
    names = {}
    if spans.trace_ids is None and trace_file is not None:
        from .decode import trace_ids_by_hash

        hexes = {t for table, r in picked for t in table.trace_ids(spans, r)}
        names = {f"{h:016x}": s
                 for h, s in trace_ids_by_hash(trace_file, (int(t, 16) for t in hexes)).items()}
    for entry in out.values():
        for e in entry.values():
            if e is not None:
                table, r = e["calls"]
                e["calls"] = _exemplar_calls(table, spans, r, names)
    return {"k": int(ex.k), "services": out}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m anomod")
    sub = ap.add_subparsers(dest="cmd", required=True)
    f = sub.add_parser("features", help="edge table + anomaly scores + ranking of one experiment")
    f.add_argument("traces", help="Jaeger all_traces.json / SkyWalking payload (file or dir)")
    f.add_argument("--metrics", help="SN metric dir (one CSV per query) or TT long metric CSV")
    f.add_argument("--window", type=int, default=60)
    f.add_argument("--alpha", type=float, default=0.85, help="PageRank damping")
    f.add_argument("--trace-step", type=float, metavar="SECONDS",
                   help="also score per-edge time series of the spans' start times, in "
                        "windows of this many seconds")
    f.add_argument("--trace-quantile", type=int, metavar="PCT",
                   help="with --trace-step: also score each edge's exact per-window latency "
                        "quantile of this percentage (0..99, e.g. 99)")
    f.add_argument("--trace-load", action="store_true",
                   help="with --trace-step: also score each edge's per-window busy time (how "
                        "long its calls were open inside every window, so calls that pile up "
                        "show in every window they last through) and write it as \"edge_load\"")
    f.add_argument("--self-time", action="store_true",
                   help="also compute the self-time (exclusive latency) edge table and "
                        "write it as \"self_edges\"")
    f.add_argument("--spectrum", action="store_true",
                   help="also label the traces abnormal / normal and write the per-service "
                        "trace coverage and Ochiai coefficients as \"spectrum\"")
    f.add_argument("--critical-path", action="store_true",
                   help="also compute the critical-path edge table (the spans that determined "
                        "each trace's end-to-end latency and the exclusive time each added; "
                        "needs span start times) and write it as \"cp_edges\"")
    f.add_argument("--shapes", action="store_true",
                   help="also take the trace shape census (the distinct call trees of the run "
                        "and how many traces have each; against --baseline, which shapes are "
                        "new) and write it as \"shapes\"")
    f.add_argument("--error-origins", action="store_true",
                   help="also tell the error-flagged spans whose failure started there from "
                        "those that relayed a callee's failure, score services by the failures "
                        "that started in them, and write the counts as \"error_origins\"")
    f.add_argument("--repeats", action="store_true",
                   help="also count, per edge, how often one parent span called the same "
                        "callee more than once (retries, retry storms, N+1 loops), score the "
                        "growth of that amplification against --baseline, and write the "
                        "counts as \"call_repeats\"")
    f.add_argument("--transit", action="store_true",
                   help="also measure, per edge, the time between two services (the request "
                        "gap from a client span's start to the callee's start and the response "
                        "gap back; needs span start times), count the calls the caller "
                        "abandoned and those that show clock skew, score the growth of the "
                        "gaps against --baseline, and write it as \"call_transit\"")
    f.add_argument("--exemplars", type=int, metavar="K",
                   help="also list, for each of the top 5 ranked services, the K slowest calls "
                        "of its slowest incoming edge and the K slowest failed calls of its "
                        "most failing one, with their trace ids, as \"exemplars\" (K in 1..64)")
    f.add_argument("--symptom-corr", action="store_true",
                   help="with --trace-step: correlate every edge's latency series and every "
                        "metric series with the front-door latency series and write the "
                        "per-service result as \"symptom_corr\" and the ten strongest "
                        "columns as \"symptom_correlates\"")
    f.add_argument("--walk", choices=("calls", "correlation"), default="calls",
                   help="what weights the ranking's walk: call counts, or (with "
                        "--symptom-corr) how each service follows the front-door latency")
    f.add_argument("--baseline", metavar="TRACES",
                   help="trace file (or dir) of a normal run: its features are the baseline "
                        "of the latency term and of the spectrum's latency thresholds")
    f.add_argument("--out", help="output JSON (default: stdout)")
    j = sub.add_parser("jaeger-to-csv",
                       help="span CSV identical to jaeger_to_csv.py's (collect_trace.sh:70)")
    j.add_argument("input")
    j.add_argument("output")
    args = ap.parse_args(argv)
    if args.cmd == "jaeger-to-csv":
        from .writers import jaeger_to_csv
        return jaeger_to_csv(args.input, args.output)

    if args.trace_load and args.trace_step is None:
        ap.error("--trace-load needs --trace-step")
    if args.symptom_corr and args.trace_step is None:
        ap.error("--symptom-corr needs --trace-step")
    if args.walk == "correlation" and not args.symptom_corr:
        ap.error("--walk correlation needs --symptom-corr")
    exp = load_experiment(args.traces, metrics=args.metrics)
    baseline = None
    if args.baseline:
        baseline = features(load_experiment(args.baseline), W=args.window,
                            self_time=args.self_time, critical_path=args.critical_path,
                            shapes=args.shapes, repeats=args.repeats, transit=args.transit)
    feats = features(exp, W=args.window, trace_step_s=args.trace_step,
                     self_time=args.self_time, baseline=baseline, spectrum=args.spectrum,
                     critical_path=args.critical_path, trace_quantile=args.trace_quantile,
                     shapes=args.shapes, error_origins=args.error_origins,
                     trace_load=args.trace_load, exemplars=args.exemplars,
                     symptom_corr=args.symptom_corr, repeats=args.repeats,
                     transit=args.transit)
    ranking = rank(feats, walk=args.walk, alpha=args.alpha)
    doc = {
        "experiment": exp.name,
        "label": exp.label,
        "services": feats.edges.services,
        "spans": exp.spans.n_spans,
        "traces": exp.spans.n_traces,
        "edges": feats.edges.records(),
        "service_scores": dict(zip(feats.edges.services, map(float, feats.service_scores))),
        "ranking": ranking,
    }
    if feats.trace_window_scores is not None:
        doc["trace_window_scores"] = dict(zip(feats.edges.services,
                                              map(float, feats.trace_window_scores)))
    if feats.self_edges is not None:
        doc["self_edges"] = feats.self_edges.records()
    if feats.cp_edges is not None:
        doc["cp_edges"] = feats.cp_edges.records()
        doc["latency_kind"] = feats.params["components"]["latency_kind"]
    if feats.spectrum is not None:
        sp = feats.spectrum
        names = feats.edges.services
        doc["spectrum"] = {
            "thresholds": feats.params["components"]["spectrum_thresholds"],
            "traces": {"normal": int(sp.n_traces[0]), "abnormal": int(sp.n_traces[1])},
            "service_traces": {s: {"normal": int(sp.svc_traces[0, i]),
                                   "abnormal": int(sp.svc_traces[1, i])}
                               for i, s in enumerate(names)},
            "ochiai": dict(zip(names, map(float, sp.ochiai()))),
        }
    if feats.shapes is not None:
        doc["shapes"] = shapes_doc(feats.shapes, exp.spans,
                                   baseline.shapes if baseline is not None else None)
    if feats.error_origins is not None:
        doc["error_origins"] = error_origins_doc(feats.error_origins)
        doc["loop_spans"] = int(feats.error_origins.loop_spans)
    if feats.repeats is not None:
        doc["call_repeats"] = call_repeats_doc(feats.repeats)
    if feats.transit is not None:
        doc["call_transit"] = call_transit_doc(feats.transit)
    if feats.edge_load is not None:
        doc["edge_load"] = edge_load_doc(feats.edge_load)
        doc["load_scores"] = dict(zip(feats.edges.services,
                                      map(float, feats.params["components"]["load"])))
    if feats.symptom_corr is not None:
        doc["symptom_corr"] = dict(zip(feats.edges.services,
                                       map(float, feats.symptom_corr.service)))
        doc["symptom_correlates"] = symptom_correlates_doc(feats.symptom_corr)
    if feats.exemplars is not None:
        doc["exemplars"] = exemplars_doc(feats, exp.spans, ranking,
                                         trace_file=exp.meta.get("trace_file"))
    text = json.dumps(doc, indent=2)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    else:
        print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
