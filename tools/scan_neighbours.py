#!/usr/bin/env python3
"""From a rocprofv3 --kernel-trace rocpd database of a bench.py run: how the other batch's purge and first pass run beside the scan.
    python tools/scan_neighbours.py <results.db> [label] [launches]
The last `launches` (default 10) long launches of the 16-wave scan make the window.  Printed: the scan's launch time, the share of the
window that scan launches cover, and per kernel of the purge and the first pass -- calls in the window, stream time per scan launch, mean
duration, how many began inside a scan launch, how many also ended inside it, and the mean duration of those that did not / did
(the tables of profiles/scan_persistent_beside_first_pass.txt and profiles/table_priority_*.txt)."""
import sqlite3
import sys

NEIGHBOURS = ("bucket_count_kernel", "split_hist_kernel", "split_scatter_kernel", "emit_bucket_rows_kernel", "emit_rescued_p_kernel",
              "rescue_count_p_kernel", "purge_detect_kernel", "purge_fix_kernel", "gather_prefix_kernel", "hll_merge_kernel", "mark_starts_kernel",
              "scan_reduce_kernel", "scan_apply_kernel", "scan_small_kernel")


def main(path: str, label: str = "", n_last: int = 10) -> None:
    cur = sqlite3.connect(path).cursor()
    ks = {r[0]: r[1] for r in cur.execute("select id, kernel_name from rocpd_info_kernel_symbol")}
    rows = [(ks.get(k, str(k)), s, e) for k, s, e in cur.execute("select kernel_id, start, end from rocpd_kernel_dispatch order by start")]
    scans = [r for r in rows if "scan_fast_kernel" in r[0]]
    if not scans:
        print(f"## {label}: no scan launch among {len(rows)} dispatches")
        return
    longest = max(e - s for _, s, e in scans)
    long_scans = [r for r in scans if r[2] - r[1] > longest / 2][-n_last:]
    t0, t1 = long_scans[0][1], long_scans[-1][2]
    d = sorted((e - s) / 1e6 for _, s, e in long_scans)
    covered = sum(e - s for _, s, e in long_scans)
    print(f"## {label}: {len(rows)} dispatches, {len(scans)} scan launches, the last {len(long_scans)} long ones taken")
    print(f"scan launch ms: median {d[len(d) // 2]:.2f} min {d[0]:.2f} max {d[-1]:.2f}")
    print(f"window {(t1 - t0) / 1e6:.1f} ms for {len(long_scans)} launches = {(t1 - t0) / 1e6 / len(long_scans):.2f} ms a launch; scans cover {100.0 * covered / (t1 - t0):.1f} % of it")
    print(f"{'kernel':48s} {'calls':>6} {'ms/launch':>10} {'avg_us':>10} {'begin in':>9} {'begin+end in':>13} {'alone_us':>9} {'inside_us':>10}")
    tenths = [0] * 10
    names = sorted({r[0] for r in rows if any(n in r[0] for n in NEIGHBOURS)})
    for name in names:
        mine = [r for r in rows if r[0] == name and r[1] >= t0 and r[2] <= t1]
        if not mine:
            continue
        begin_in, both_in, alone, inside = 0, 0, [], []
        for _, s, e in mine:
            host = next((sc for sc in long_scans if sc[1] <= s < sc[2]), None)
            if host is not None:
                begin_in += 1
                if "split_" in name or "bucket_count" in name:
                    tenths[min(9, int(10 * (s - host[1]) / (host[2] - host[1])))] += 1
            if host is not None and e <= host[2]:
                both_in += 1
                inside.append(e - s)
            else:
                alone.append(e - s)
        total = sum(e - s for _, s, e in mine)
        mean = lambda v: sum(v) / len(v) / 1e3 if v else 0.0
        print(f"{name[:48]:48s} {len(mine):6d} {total / 1e6 / len(long_scans):10.3f} {mean([e - s for _, s, e in mine]):10.1f} {begin_in:9d} {both_in:13d} "
              f"{mean(alone):9.1f} {mean(inside):10.1f}")
    print(f"split / bucket_count launches that begin in each tenth of a scan launch: {tenths}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "", int(sys.argv[3]) if len(sys.argv) > 3 else 10)
