"""CLI:  python -m anomod features <trace file|dir> [--metrics PATH] [--out FILE]
                                 [--spectrum] [--critical-path] [--shapes]
                                 [--error-origins] [--trace-step S [--trace-load]]
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
    exp = load_experiment(args.traces, metrics=args.metrics)
    baseline = None
    if args.baseline:
        baseline = features(load_experiment(args.baseline), W=args.window,
                            self_time=args.self_time, critical_path=args.critical_path,
                            shapes=args.shapes)
    feats = features(exp, W=args.window, trace_step_s=args.trace_step,
                     self_time=args.self_time, baseline=baseline, spectrum=args.spectrum,
                     critical_path=args.critical_path, trace_quantile=args.trace_quantile,
                     shapes=args.shapes, error_origins=args.error_origins,
                     trace_load=args.trace_load)
    ranking = rank(feats, alpha=args.alpha)
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
    if feats.edge_load is not None:
        doc["edge_load"] = edge_load_doc(feats.edge_load)
        doc["load_scores"] = dict(zip(feats.edges.services,
                                      map(float, feats.params["components"]["load"])))
    text = json.dumps(doc, indent=2)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    else:
        print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
