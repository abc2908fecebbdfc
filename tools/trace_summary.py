"""Summarise a rocprofv3 --kernel-trace CSV of the bench command (profiles/r07/*trace*.json).

    rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python3 bench.py --gpus 1 --steps 30 --warmup 5
    python tools/trace_summary.py DIR/.../run_kernel_trace.csv out.json

Writes per-kernel average durations over the second half of each kernel's launches (the first half holds the warm-up
and clock-settle steps), the span from the start of a frame's first preprocess kernel to the start of its k_blend_fwd
(what the forward's front costs on the critical path, whatever runs beside it), and the last frame's timeline with
each dispatch's stream id.
"""
import collections
import csv
import json
import sys


def short(name):
    return name.replace("void ", "").split("(")[0].split("::")[-1]


def main(trace, out):
    rows = list(csv.DictReader(open(trace)))
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]),
                 r.get("Stream_Id", r.get("Queue_Id", ""))) for r in rows)
    dur = collections.defaultdict(list)
    for s, e, n, _ in ev:
        dur[n].append((e - s) / 1e3)
    res = {"kernels_avg_us_second_half": {n: round(sum(v[len(v) // 2:]) / len(v[len(v) // 2:]), 2)
                                          for n, v in dur.items() if n.startswith("k_")},
           "launches": {n: len(v) for n, v in dur.items() if n.startswith("k_")}}
    first = ("k_preprocess_geom", "k_preprocess_sh2")
    spans, after_colour = [], []
    pre = colour_end = None
    for s, e, n, _ in ev:
        if n.startswith(first):
            pre, colour_end = s, None
        elif n.startswith("k_preprocess_colour"):
            colour_end = e
        elif n.startswith("k_blend_fwd") and pre is not None:
            spans.append((s - pre) / 1e3)
            if colour_end is not None:
                after_colour.append((s - colour_end) / 1e3)
            pre = None
    k = len(spans) // 2

    def stats(v):
        return {"n": len(v), "avg": round(sum(v) / max(1, len(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    res["pre_start_to_blend_fwd_start_us"] = stats(spans[k:])
    if after_colour:
        res["blend_start_minus_colour_end_us"] = stats(after_colour[k:])
    last = [i for i, x in enumerate(ev) if x[2].startswith(first)][-1]
    t0 = ev[last][0]
    res["last_frame_timeline_us"] = [[n, q, round((s - t0) / 1e3, 1), round((e - t0) / 1e3, 1)]
                                     for s, e, n, q in ev[last:last + 14]]
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(*sys.argv[1:3])
