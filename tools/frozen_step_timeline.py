"""One settled step of the frozen-manifold cfg2 run out of a rocprofv3 kernel trace (CSV), every queue, in the format of
profiles/r07_frozen_step_timeline.txt, followed by the three figures the broad-phase placement is judged by:
  - where k_update_aabb starts relative to the step's first k_body_warm_start and first k_integrate_positions,
  - the idle gap in front of k_writeback_solver_bodies (and the largest other gap on the world's queue),
  - the mean colour launch overlapped / not overlapped by a kernel of another queue (whole trace).

    python tools/frozen_step_timeline.py <kernel_trace.csv> [step index, default 40]
"""
import csv
import sys


def short(name):
    return name.split("(")[0].replace("void avn::", "").replace("avn::", "")[:56]


def is_colour(name):
    return "k_color_pass" in name or "k_overflow" in name


def main():
    path = sys.argv[1]
    which = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], short(r["Kernel_Name"]),
                     int(r.get("Grid_Size", 0) or 0)))
    rows.sort()
    # a step = from one k_prepare_solver_bodies (the front's first kernel) to the next
    fronts = [i for i, r in enumerate(rows) if "k_prepare_solver_bodies" in r[3]]
    if len(fronts) < which + 2:
        which = len(fronts) - 2
    a, b = rows[fronts[which]][0], rows[fronts[which + 1]][0]
    step = [r for r in rows if a <= r[0] < b]
    # the broad phase of this step may have started before the front's first kernel only if it was enqueued first; include what overlaps
    wq = rows[fronts[which]][2]
    queues = {}
    for r in step:
        queues[r[2]] = queues.get(r[2], 0) + 1
    print("queues (id: kernels):", queues)
    t0 = a
    last_end = {}
    out = []
    group = []

    def flush():
        if group:
            n = len(group)
            d = sum(e - s for s, e, *_ in group) / n / 1e3
            out.append((group[0][0], "%9.1f us  +%8.1f us  q%s [%d x colour/overflow] mean %.2f us" % ((group[0][0] - t0) / 1e3, (group[-1][1] - group[0][0]) / 1e3, group[0][2], n, d)))
            group.clear()

    gaps = []
    for r in step:
        s, e, q, name, grid = r
        gap = max(0.0, (s - last_end[q]) / 1e3) if q in last_end else 0.0
        last_end[q] = max(last_end.get(q, 0), e)
        if q == wq:
            gaps.append((gap, name))
        if is_colour(name) and q == wq:
            group.append(r)
            continue
        if q == wq:
            flush()
        out.append((s, "%9.1f us  +%8.1f us  gap %7.1f  q%s %s  [%d]" % ((s - t0) / 1e3, (e - s) / 1e3, gap, q, name, grid)))
    flush()
    print("\n".join(line for _, line in sorted(out)))
    print("step span %.1f us" % ((b - a) / 1e3))

    def first(sub):
        for r in step:
            if sub in r[3]:
                return r
        return None

    ua, ws, ip, wb = first("k_update_aabb"), first("k_body_warm_start"), first("k_integrate_positions"), first("k_writeback_solver_bodies")
    if ua and ws and ip:
        print("k_update_aabb starts %+.1f us from the first k_body_warm_start, %+.1f us from the first k_integrate_positions" % ((ua[0] - ws[0]) / 1e3, (ua[0] - ip[0]) / 1e3))
    if wb:
        g = [x for x in gaps if "k_writeback_solver_bodies" in x[1]]
        others = sorted((x for x in gaps if "k_writeback_solver_bodies" not in x[1]), reverse=True)
        print("gap in front of k_writeback_solver_bodies %.1f us; largest other gap on its queue %.1f us (%s)" % (g[0][0] if g else -1.0, others[0][0], others[0][1]))
    sw = first("k_sweep<")
    if sw:
        print("k_sweep %.1f us  [%d]" % ((sw[1] - sw[0]) / 1e3, sw[4]))
    # whole trace, settled steps only: colour launches with and without a kernel of another queue beside them
    lo = rows[fronts[min(8, len(fronts) - 1)]][0]
    others = sorted((r[0], r[1]) for r in rows if r[2] != wq and r[0] >= lo)
    import bisect
    starts = [o[0] for o in others]
    ov, no = [], []
    for s, e, q, name, _ in rows:
        if q != wq or s < lo or not is_colour(name):
            continue
        k = bisect.bisect_left(starts, e)
        hit = any(o[1] > s for o in others[max(0, k - 24):k])
        (ov if hit else no).append((e - s) / 1e3)
    if no:
        print("colour launches not overlapped: %d  mean %.2f us" % (len(no), sum(no) / len(no)))
    if ov:
        print("colour launches overlapped by another queue: %d  mean %.2f us" % (len(ov), sum(ov) / len(ov)))


if __name__ == "__main__":
    main()
