"""Per-sweep span from a rocprofv3 kernel_trace.csv: the sweep kernels
(k_sweep_flatw, k_sweep_tiled, k_sweep_ubands or the k_sweep_bands launches)
may run on several streams and overlap, so rocprof's per-kernel averages are
concurrent spans; the sweep's duration is max(end) - min(start) over its
dispatches, grouped by the k_marg that follows each sweep.  Per kernel name the
mean start and end within its sweep (ms from the sweep's first start) show the
schedule: which kernels overlap, which ends last, and how long the phase of
the kernels that are not the flat one takes (second_phase_ms: from the first
start to the last end among them).
python tools/sweep_span.py <trace.csv> <out.json>"""
import csv
import json
import sys


def short(name):
    return name.replace("void ", "").split("<")[0].split("(")[0].split("::")[-1]


def main(path, out):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    sweeps, cur = [], []
    for r in rows:
        name = r["Kernel_Name"]
        if "k_sweep_" in name:
            cur.append((short(name), int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
        elif "k_marg" in name and cur:
            sweeps.append(cur)
            cur = []
    spans = [(max(e for _, _, e in sw) - min(s for _, s, _ in sw)) / 1e6 for sw in sweeps]
    kern, second = {}, []
    for sw in sweeps:
        t0 = min(s for _, s, _ in sw)
        for k in {k for k, _, _ in sw}:
            mine = [(s, e) for kk, s, e in sw if kk == k]
            acc = kern.setdefault(k, [0.0, 0.0, 0.0, 0])
            acc[0] += (min(s for s, _ in mine) - t0) / 1e6
            acc[1] += (max(e for _, e in mine) - t0) / 1e6
            acc[2] += sum(e - s for s, e in mine) / 1e6
            acc[3] += 1
        rest = [(s, e) for k, s, e in sw if "flat" not in k]
        if rest:
            second.append((max(e for _, e in rest) - min(s for s, _ in rest)) / 1e6)
    res = {"sweeps": len(spans), "span_ms_avg": sum(spans) / max(len(spans), 1),
           "span_ms_min": min(spans) if spans else None, "span_ms_max": max(spans) if spans else None,
           "second_phase_ms": sum(second) / len(second) if second else None,
           "kernels": {k: {"start_ms": round(a[0] / a[3], 4), "end_ms": round(a[1] / a[3], 4),
                           "busy_ms": round(a[2] / a[3], 4)} for k, a in sorted(kern.items())}}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
