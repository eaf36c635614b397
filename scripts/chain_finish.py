"""Reader of tools/chain_check's finish table (`chain_check time 4096`, a profiling build): the
"simd" rows give, per (XCC, SE, SH, CU, SIMD), its waves' slots and their finish times as fractions
of the kernel, sorted.  Every wave has the same work, so the spread inside a SIMD is the
instruction arbiter's and the spread between SIMDs is placement.  Prints, over the SIMDs that held
four waves: the mean finish fraction of each rank, of all waves (the residency ratio
R = 4 SQ_WAVE_CYCLES / SQ_WAVES / (GRBM_GUI_ACTIVE / 8) of the counters), the mean spread inside a
SIMD against the spread of the last finisher between SIMDs, and the mean finish by wave slot (which
slot the arbiter favours).  usage: python3 scripts/chain_finish.py FILE [FILE ...]"""
import re
import statistics
import sys

ROW = re.compile(r"^simd xcc (\d+) se (\d+) sh (\d+) cu\s+(\d+) simd (\d+) waves (\d+) slots ([\d ]+) finish ([\d. ]+)$")


def read(path):
    simds = []
    head = ""
    for line in open(path):
        if line.startswith(("chain ", "(workspace")):
            head = line.strip()
        m = ROW.match(line.strip())
        if m:
            slots = [int(x) for x in m.group(7).split()]
            fin = [float(x) for x in m.group(8).split()]
            simds.append((int(m.group(1)), slots, fin))
    return head, simds


for path in sys.argv[1:]:
    head, simds = read(path)
    four = [s for s in simds if len(s[2]) == 4]
    print(f"{path}: {head.split(';')[0]}")
    if not four:
        print("  no SIMD with four waves")
        continue
    ranks = [statistics.fmean(s[2][r] for s in four) for r in range(4)]
    inside = statistics.fmean(s[2][3] - s[2][0] for s in four)
    last = [s[2][3] for s in four]
    by_slot = {}
    for _, slots, fin in four:
        for k, f in zip(slots, fin):
            by_slot.setdefault(k, []).append(f)
    print(f"  {len(four)} SIMDs with four waves of {len(simds)}")
    print("  mean finish fraction by rank: " + " ".join(f"{r:.3f}" for r in ranks)
          + f"; of all waves {statistics.fmean(ranks):.3f}")
    print(f"  spread inside a SIMD (last - first) {inside:.3f}; last finisher between SIMDs: "
          f"min {min(last):.3f} max {max(last):.3f} sd {statistics.pstdev(last):.3f}")
    print("  mean finish fraction by wave slot: "
          + " ".join(f"{k}: {statistics.fmean(v):.3f}" for k, v in sorted(by_slot.items())))
    xcc = {}
    for x, _, fin in four:
        xcc.setdefault(x, []).append(fin[3])
    print("  last finisher by XCC: " + " ".join(f"{x}: {statistics.fmean(v):.3f}" for x, v in sorted(xcc.items())))
