"""Device time of one SLAM chunk from a rocprofv3 kernel trace (the timed region, after the last torch kernel).

A chunk is the update chain's run of launches from a k_feature to the next k_chain_apply that holds a k_ekf_MS and
a k_ekf_WP (the direct update of a small batch: in cfg3 / cfg3t these are UpdaterSLAM::update's chunks; the MSCKF
update there is the information form and a delayed-initialization candidate uses k_di_M).  Its device time is the
sum of the durations of the chain's own kernels (other streams' kernels that fall inside the window are left out);
the window (first start to last end) is printed too.
usage: slam_chunk_time.py trace.csv"""
import collections
import csv
import sys

CHAIN = ("k_feature", "k_gemm_HPg", "k_chi2", "k_ekf_MS", "k_ekf_fact", "k_ekf_WP", "k_chain_apply")


def short(n):
    return n.split('(')[0].replace('uvhp::', '').replace('void ', '')


rows = list(csv.DictReader(open(sys.argv[1])))
ev = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name'])) for r in rows)
last_torch = max([i for i, e in enumerate(ev) if 'at::' in e[2]] + [-1])
seg = [e for e in ev[last_torch + 1:] if e[2].startswith(CHAIN)]
chunks, cur = [], None
for e in seg:
    if e[2].startswith("k_feature"):
        cur = [e]
    elif cur is not None:
        cur.append(e)
        if e[2].startswith("k_chain_apply"):
            names = [x[2] for x in cur]
            if any(n.startswith("k_ekf_MS") for n in names) and any(n.startswith("k_ekf_WP") for n in names):
                chunks.append(cur)
            cur = None
if not chunks:
    sys.exit("no SLAM chunk in the trace")
dev = [sum(e[1] - e[0] for e in c) / 1e3 for c in chunks]
win = [(c[-1][1] - c[0][0]) / 1e3 for c in chunks]
dev.sort()
print("SLAM chunks %d  launches per chunk %.2f  device time per chunk: mean %.1f us  median %.1f us  "
      "window mean %.1f us" % (len(chunks), sum(len(c) for c in chunks) / len(chunks), sum(dev) / len(dev),
                               dev[len(dev) // 2], sum(win) / len(win)))
per = collections.defaultdict(list)
for c in chunks:
    for s, e, n in c:
        per[n].append((e - s) / 1e3)
for n in sorted(per, key=lambda k: -sum(per[k])):
    print("  %-28s per chunk %5.2f  avg %6.1f us  per chunk %6.1f us" % (n[:28], len(per[n]) / len(chunks),
                                                                      sum(per[n]) / len(per[n]),
                                                                      sum(per[n]) / len(chunks)))
