"""Timeline of the instance-minor evaluation's kernels from a rocprofv3 --kernel-trace CSV.

    python tools/soa_timeline.py TRACE_kernel_trace.csv [--steps 50] [--label TEXT]

An evaluation (a step of bench.py) ends with ap2_finalize_kernel; the node kernels before it are
ap2_soa_eval_kernel (one launch) or ap2_soa_radau_kernel + ap2_soa_shoot_kernel (two streams).
Prints a markdown table over the last --steps evaluations of the trace (the timed ones: the warm-up
comes first): start and end of every kernel relative to the evaluation's first kernel start, the
span to the finalize kernel's end, and the idle gaps between the kernels and to the next
evaluation.  Median, minimum and maximum, in microseconds."""
import argparse
import csv
import statistics
import sys

NODE = ("ap2_soa_eval_kernel", "ap2_soa_radau_kernel", "ap2_soa_shoot_kernel")
FINAL = "ap2_finalize_kernel"


def read(path):
    rows = []
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        kind = next((k for k in NODE + (FINAL,) if k in name), None)
        if kind:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind))
    rows.sort()
    return rows


def evaluations(rows):
    """[{kind: (start, end)}] per evaluation: the kernels up to and including a finalize kernel."""
    out, cur = [], {}
    for s, e, kind in rows:
        cur[kind] = (s, e)
        if kind == FINAL:
            if any(k in cur for k in NODE):
                out.append(cur)
            cur = {}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    evs = evaluations(read(a.trace))
    # the timed steps of one bench.py run are back to back: keep the last --steps evaluations that
    # have the same kernels as the last one
    evs = [e for e in evs if set(e) == set(evs[-1])][-a.steps:]
    if len(evs) < 2:
        sys.exit("fewer than two evaluations in the trace")
    cols = {}

    def put(key, v):
        cols.setdefault(key, []).append(v / 1e3)

    for i, e in enumerate(evs):
        nodes = [k for k in NODE if k in e]
        t0 = min(e[k][0] for k in nodes)
        for k in nodes:
            put(k + " start", e[k][0] - t0)
            put(k + " end", e[k][1] - t0)
            put(k + " duration", e[k][1] - e[k][0])
        if "ap2_soa_shoot_kernel" in e and "ap2_soa_radau_kernel" in e:
            put("gap: shoot start - Radau start", e["ap2_soa_shoot_kernel"][0] - e["ap2_soa_radau_kernel"][0])
            put("Radau end - shoot end (Radau tiles alone)", e["ap2_soa_radau_kernel"][1] - e["ap2_soa_shoot_kernel"][1])
        node_end = max(e[k][1] for k in nodes)
        put(FINAL + " start", e[FINAL][0] - t0)
        put(FINAL + " end = span", e[FINAL][1] - t0)
        put(FINAL + " duration", e[FINAL][1] - e[FINAL][0])
        put("gap: last node kernel end -> finalize start", e[FINAL][0] - node_end)
        if i + 1 < len(evs):
            nxt = evs[i + 1]
            n0 = min(nxt[k][0] for k in NODE if k in nxt)
            put("gap: finalize end -> next evaluation's first kernel", n0 - e[FINAL][1])
            put("period: first kernel start -> next evaluation's", n0 - t0)
    print("### %s" % (a.label or a.trace))
    print()
    print("%d evaluations, microseconds relative to the evaluation's first kernel start" % len(evs))
    print()
    print("| | median | min | max |")
    print("|---|---|---|---|")
    for k, v in cols.items():
        print("| %s | %.1f | %.1f | %.1f |" % (k, statistics.median(v), min(v), max(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
