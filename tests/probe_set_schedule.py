"""A host model of how jpegx_probe_sizes_set_n deals its work: tests/probe_schedule.py's turn loop with the plane of a block
taken from a list of plane starts instead of a division -- k_probe_n<true> restated in plain Python, with nothing of the
product imported.  tests/test_gpu_probe_set_scale_n.py takes its shapes (SCALE) and the block of a carried turn from here;
tests/test_probe_set_schedule.py holds the shapes against the model.

  starts  the first block of every plane and, last, the block count: strictly ascending, starts[0] = 0
  plane(g) = the p with starts[p] <= g < starts[p + 1]: monotone in g, and a step of one block raises it by one at most

A turn holds the blocks first .. first + nlive - 1 of the planes plane0 .. plane0 + rows - 1, plane0 = plane(first); `leave` is
true on the last turn of a run, or when plane(first of the next turn) != plane0.  A turn that does not leave lies inside
plane0 (monotone: plane0 = plane(first) <= plane(g) <= plane(next first) = plane0), so rows = 1 and row 0 is carried."""
from bisect import bisect_right

from probe_schedule import Turn, blocks_per_wg, constant_of, events  # noqa: F401  (events works on any schedule with runs())

# N -> (the cycle of blocks per plane, planes, the run intended): unequal planes whose ends fall at every phase of a turn
SCALE = {
    2: ((225, 1, 1, 383, 64, 65, 7, 130, 1, 200, 3, 449), 4125, 2),      # 64 blocks a turn, 8209 turns
    4: ((63, 1, 100, 5, 37, 150, 16, 17, 1, 81), 5570, 3),               # 16 blocks a turn, 16 397 turns
    17: ((1, 5, 2, 1, 7, 3, 4), 2496, 2),                                # a block a turn, 8197 turns
}


def starts_of(counts):
    out = [0]
    for c in counts:
        assert c >= 1
        out.append(out[-1] + int(c))
    return out


def scale_counts(n):
    cycle, nplanes, _ = SCALE[n]
    return [cycle[p % len(cycle)] for p in range(nplanes)]


class SetSchedule:
    def __init__(self, n, starts, threads, max_workgroups):
        assert starts[0] == 0 and all(b > a for a, b in zip(starts, starts[1:]))
        self.n, self.starts, self.nplanes = n, list(starts), len(starts) - 1
        self.bpw = blocks_per_wg(n, threads)
        self.nblk = starts[-1]
        self.nturns = -(-self.nblk // self.bpw)
        self.run = -(-self.nturns // max_workgroups)
        self.grid = -(-self.nturns // self.run)

    def plane_of(self, block):
        return bisect_right(self.starts, block) - 1

    def turns_of(self, wg):
        """The turns of workgroup wg in order."""
        turn0 = wg * self.run
        turn1 = min(turn0 + self.run, self.nturns)
        out = []
        for turn in range(turn0, turn1):
            first = turn * self.bpw
            nlive = min(self.bpw, self.nblk - first)
            plane0 = self.plane_of(first)
            rows = self.plane_of(first + nlive - 1) - plane0 + 1
            leave = turn + 1 == turn1 or self.plane_of((turn + 1) * self.bpw) != plane0
            out.append(Turn(turn, wg, first, nlive, plane0, rows, leave))
        return out

    def runs(self):
        return [self.turns_of(wg) for wg in range(self.grid)]

    def turn_of_block(self, block):
        t = block // self.bpw
        return self.turns_of(t // self.run)[t % self.run]


def scale_schedule(n):
    return SetSchedule(n, starts_of(scale_counts(n)), constant_of("jpegx_dctn_device.h", "DCTN_THREADS"),
                       constant_of("jpegx_probe_n.hip", "PROBE_MAX_WORKGROUPS"))


def plane_end_after(s, t):
    """The end (a block index) of the plane in which turn t starts."""
    return s.starts[t.plane0 + 1]


def simulate(s, weight, clear=True, leave_against=0):
    """The totals per plane that the ragged turn loop gives when block g weighs weight[g].  clear False (the sums are not
    cleared after they went out) and leave_against 1 (`leave` compares the next turn's plane against plane0 + 1) are the two
    defects of probe_schedule.simulate, kept so that the schedule test can show that a shape would notice them."""
    before = [0]
    for w in weight:
        before.append(before[-1] + int(w))
    totals = [0] * s.nplanes
    for turns in s.runs():
        acc = [0] * s.bpw
        turn1 = turns[-1].turn + 1
        for t in turns:
            for e in range(t.rows):                            # the turn's blocks of plane plane0 + e
                lo, hi = max(t.first, s.starts[t.plane0 + e]), min(t.first + t.nlive, s.starts[t.plane0 + e + 1])
                acc[e] += before[hi] - before[lo]
            nxt = (t.turn + 1) * s.bpw
            leave = t.turn + 1 == turn1 or (s.plane_of(nxt) if nxt < s.nblk else -1) != t.plane0 + leave_against
            if leave:
                for e in range(t.rows):
                    totals[t.plane0 + e] += acc[e]
                    if clear:
                        acc[e] = 0
    return totals


def carried_block(s):
    """(plane, block of the strip) of a block in a CARRIED turn of the middle of the grid."""
    carries = events(s)["carry"]
    wg, turn = carries[len(carries) // 2]
    t = s.turns_of(wg)[turn - wg * s.run]
    assert t.turn == turn and not t.leave and t.rows == 1
    block = t.first + t.nlive // 2
    assert s.plane_of(block) == t.plane0
    return t.plane0, block
