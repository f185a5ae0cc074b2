"""A host model of how jpegx_probe_sizes_n deals its work: the launcher's arithmetic and k_probe_n's turn loop restated in plain
Python, with nothing of the product imported.  tests/test_gpu_probe_scale_n.py holds its shapes against it and picks from it
the plane and the block of a carried turn.

  bpw     blocks per turn: dctn_blocks_per_wg(N) = 1 for N^2 >= DCTN_THREADS, DCTN_THREADS / N^2 otherwise
  nturns  ceil(blocks / bpw)              run  ceil(nturns / PROBE_MAX_WORKGROUPS) turns per workgroup
  grid    ceil(nturns / run) workgroups; workgroup w owns the turns w * run .. min((w + 1) * run, nturns) - 1

A turn holds the blocks first .. first + nlive - 1 (first = turn * bpw), of the planes plane0 .. plane0 + rows - 1; the
workgroup adds the sums it holds to the totals and clears them when `leave` is true: on the last turn of its run, or when the
next turn starts in another plane than this one did.  Otherwise the turn lay inside one plane and its row 0 is the next
turn's row 0: a CARRY."""
import os
import re
from collections import namedtuple

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "implementing-jpeg-compression_amd", "csrc")

Turn = namedtuple("Turn", "turn wg first nlive plane0 rows leave")


def constant_of(source, name):
    """An integer `constexpr` of a source file of the library, read with a regular expression."""
    with open(os.path.join(CSRC, source)) as f:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert m, "%s is no longer defined in %s" % (name, source)
    return int(m.group(1))


def blocks_per_wg(n, threads):
    return 1 if n * n >= threads else threads // (n * n)


class Schedule:
    def __init__(self, n, nplanes, bpp, threads, max_workgroups):
        self.n, self.nplanes, self.bpp = n, nplanes, bpp
        self.bpw = blocks_per_wg(n, threads)
        self.nblk = nplanes * bpp
        self.nturns = -(-self.nblk // self.bpw)
        self.run = -(-self.nturns // max_workgroups)
        self.grid = -(-self.nturns // self.run)

    def turns_of(self, wg):
        """The turns of workgroup wg in order."""
        turn0 = wg * self.run
        turn1 = min(turn0 + self.run, self.nturns)
        out = []
        for turn in range(turn0, turn1):
            first = turn * self.bpw
            nlive = min(self.bpw, self.nblk - first)
            plane0 = first // self.bpp
            rows = (first + nlive - 1) // self.bpp - plane0 + 1
            leave = turn + 1 == turn1 or ((turn + 1) * self.bpw) // self.bpp != plane0
            out.append(Turn(turn, wg, first, nlive, plane0, rows, leave))
        return out

    def runs(self):
        return [self.turns_of(wg) for wg in range(self.grid)]

    def turn_of_block(self, block):
        t = block // self.bpw
        return self.turns_of(t // self.run)[t % self.run]


def events(s):
    """Which of the things a run of several turns can do happen in schedule s: name -> the (workgroup, turn) pairs where.

      carry           a turn inside one plane that does not leave: the next turn, in the same plane, inherits row 0
      carry_twice     two such turns in a row (run >= 3)
      flush_then_on   a turn that leaves without being the last of its run: what follows needs the cleared sums
      straddle_first  the first turn of a run of several holds blocks of more than one plane
      straddle_later  a later turn of a run does
      short_last      the last workgroup has fewer than `run` turns"""
    found = {k: [] for k in ("carry", "carry_twice", "flush_then_on", "straddle_first", "straddle_later", "short_last")}
    for turns in s.runs():
        for i, t in enumerate(turns):
            at = (t.wg, t.turn)
            if not t.leave:
                assert t.rows == 1 and i + 1 < len(turns) and turns[i + 1].plane0 == t.plane0
                found["carry"].append(at)
                if i > 0 and not turns[i - 1].leave:
                    found["carry_twice"].append(at)
            elif i + 1 < len(turns):
                found["flush_then_on"].append(at)
            if t.rows > 1 and len(turns) > 1:
                found["straddle_first" if i == 0 else "straddle_later"].append(at)
    last = s.turns_of(s.grid - 1)
    if len(last) < s.run:
        found["short_last"].append((s.grid - 1, last[-1].turn))
    return found


def simulate(s, weight, clear=True, leave_against=0):
    """The totals per plane that the turn loop gives when block g weighs weight[g]: the table of sums per workgroup, filled turn
    by turn, added to the totals and cleared where the kernel does so.  clear False and leave_against 1 are the two defects of
    tests/test_gpu_probe_scale_n.py's docstring, kept here so that the premises test can show that a shape would notice them."""
    before = [0]                                           # before[g]: the weight of the blocks in front of g
    for w in weight:
        before.append(before[-1] + int(w))
    totals = [0] * s.nplanes
    for turns in s.runs():
        acc = [0] * s.bpw
        turn1 = turns[-1].turn + 1
        for t in turns:
            for e in range(t.rows):                            # the turn's blocks of plane plane0 + e
                lo, hi = max(t.first, (t.plane0 + e) * s.bpp), min(t.first + t.nlive, (t.plane0 + e + 1) * s.bpp)
                acc[e] += before[hi] - before[lo]
            leave = t.turn + 1 == turn1 or ((t.turn + 1) * s.bpw) // s.bpp != t.plane0 + leave_against
            if leave:
                for e in range(t.rows):
                    totals[t.plane0 + e] += acc[e]
                    if clear:
                        acc[e] = 0
    return totals
