#!/usr/bin/env python
"""tools/track_call_trace.py KERNEL_TRACE.csv -- head, steady state and tail of the LAST mtfhip_batch_track call in a rocprofv3 kernel trace
(`rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python bench.py --gpus 1 --steps K --warmup W`: the last call of a
plain run is the last timed region).  The figures of profiles/track_call_cost.md come from this script.

  head          first kernel of the call (the slab ingest / the prologue) -> the first pixel pass on each queue
  steady state  per queue: period (start to start of the pixel passes), duration of the pixel pass and of the finish; how much of a
                pixel pass runs beside one of the other queue
  tail          end of the last pixel pass -> end of the last kernel of the call
"""
import csv
import statistics
import sys


def short(name):
    for k in ("k_fused_ssd", "k_finish_track", "k_publish_host", "k_ingest_host", "k_track_prologue", "k_queue_delay"):
        if k in name:
            return k
    return name.split("(")[0][-40:]


def main(path):
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r.get("Queue_Id", "?")))
    rows.sort()
    fused = [i for i, r in enumerate(rows) if r[2] == "k_fused_ssd"]
    if not fused:
        raise SystemExit("no k_fused_ssd in the trace")
    heads = [i for i, r in enumerate(rows) if r[2] in ("k_ingest_host", "k_track_prologue") and any(rows[j][2] == "k_fused_ssd" for j in range(i + 1, min(i + 8, len(rows))))]
    call = rows[heads[-1]:]
    t0 = call[0][0]
    us = lambda ns: ns / 1e3
    print("call: %d kernels, %.1f us from the first kernel's start to the last kernel's end" % (len(call), us(max(r[1] for r in call) - t0)))
    print("-- first kernels (start, end in us from the call's first kernel; queue)")
    for r in call[:10]:
        print("   %8.1f %8.1f  q%-3s %s" % (us(r[0] - t0), us(r[1] - t0), r[3], r[2]))
    queues = []
    for r in call:
        if r[2] == "k_fused_ssd" and r[3] not in queues:
            queues.append(r[3])
    per_q = {q: [r for r in call if r[3] == q] for q in queues}
    for q in queues:
        f = [r for r in per_q[q] if r[2] == "k_fused_ssd"]
        fin = [r for r in per_q[q] if r[2] == "k_finish_track"]
        print("queue %s: head %.1f us; %d pixel passes, %d finishes" % (q, us(f[0][0] - t0), len(f), len(fin)))
        if len(f) > 3:
            per = [us(b[0] - a[0]) for a, b in zip(f[1:-2], f[2:-1])]   # (without the first pass and the materialising last one)
            print("   period median %.2f us (min %.2f, max %.2f)" % (statistics.median(per), min(per), max(per)))
        mid = f[1:-1] if len(f) > 2 else f
        print("   k_fused_ssd  median %.2f us (lean passes), last (materialising) %.2f us" % (statistics.median(us(r[1] - r[0]) for r in mid), us(f[-1][1] - f[-1][0])))
        if fin:
            d = [us(r[1] - r[0]) for r in fin]
            print("   k_finish_track median %.2f us (min %.2f, max %.2f)" % (statistics.median(d), min(d), max(d)))
            g1 = [us(fin[i][0] - f[i][1]) for i in range(min(len(f), len(fin)))]
            g2 = [us(f[i + 1][0] - fin[i][1]) for i in range(min(len(f) - 1, len(fin)))]
            print("   boundary pixel pass -> finish median %.2f us, finish -> next pixel pass median %.2f us" % (statistics.median(g1), statistics.median(g2) if g2 else float("nan")))
    if len(queues) == 2:
        a = [r for r in per_q[queues[0]] if r[2] == "k_fused_ssd"][1:-1]
        b = [r for r in per_q[queues[1]] if r[2] == "k_fused_ssd"][1:-1]
        ov = []
        for x in a:
            o = sum(max(0, min(x[1], y[1]) - max(x[0], y[0])) for y in b)
            ov.append(o / max(1, x[1] - x[0]))
        if ov:
            print("overlap: a pixel pass of queue %s runs beside one of queue %s for %.0f %% of its duration (median)" % (queues[0], queues[1], 100 * statistics.median(ov)))
    last_f = max(r[1] for r in call if r[2] == "k_fused_ssd")
    print("tail: %.1f us from the end of the last pixel pass to the end of the call's last kernel" % us(max(r[1] for r in call) - last_f))
    print("-- last kernels")
    for r in call[-8:]:
        print("   %8.1f %8.1f  q%-3s %s" % (us(r[0] - t0), us(r[1] - t0), r[3], r[2]))


if __name__ == "__main__":
    main(sys.argv[1])
