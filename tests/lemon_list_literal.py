"""TEST AID.  Literal restatement of LEMON's CandidateListPivotRule and AlteringListPivotRule (lemon-1.3.1/lemon/network_simplex.h:415-635),
in the spirit of oracle/bspo_literal.py, and a driver that runs them on the library's own sequential half: mcf_ns_begin -> mcf_ns_internal
(state, pi, cost, source, target, read in place) -> mcf_ns_apply_pivot(arc) per pivot -> mcf_ns_finish.  The sequential half is checked
against the oracle elsewhere; this file pins the two rules' control flow to the source, and the GPU tests then hold the device solves to it.

Statement for statement with two liberties that change no result: the arc scans of a major iteration / list extension read the reduced costs
of a run of consecutive arcs with numpy (nothing changes while a rule scans, so evaluating a run at once is the same as one arc at a time), and
LEMON's `goto search_end` is a `break` out of both loops.  std::partial_sort is libstdc++'s (bits/stl_algo.h __partial_sort = __heap_select +
__sort_heap, bits/stl_heap.h __make_heap / __adjust_heap / __push_heap / __pop_heap), which is what LEMON built with g++ runs: Python's heapq
or sorted() order equal keys differently.
"""
import ctypes as C
import math

import numpy as np

from mincostflow_amd import _lib as L

CANDIDATE_LIST, ALTERING_LIST = 3, 4
NOT_SOLVED, OPTIMAL, INFEASIBLE, UNBOUNDED = 0, 1, 2, 3


# ---------------------------------------------------------------- libstdc++'s std::partial_sort on a Python list, [first, middle, last)
def _push_heap(a, first, hole, top, value, comp):
    parent = (hole - 1) // 2
    while hole > top and comp(a[first + parent], value):
        a[first + hole] = a[first + parent]
        hole = parent
        parent = (hole - 1) // 2
    a[first + hole] = value


def _adjust_heap(a, first, hole, length, value, comp):
    top = hole
    second = hole
    while second < (length - 1) // 2:
        second = 2 * (second + 1)
        if comp(a[first + second], a[first + (second - 1)]):
            second -= 1
        a[first + hole] = a[first + second]
        hole = second
    if (length & 1) == 0 and second == (length - 2) // 2:
        second = 2 * (second + 1)
        a[first + hole] = a[first + (second - 1)]
        hole = second - 1
    _push_heap(a, first, hole, top, value, comp)


def _make_heap(a, first, last, comp):
    length = last - first
    if length < 2:
        return
    parent = (length - 2) // 2
    while True:
        value = a[first + parent]
        _adjust_heap(a, first, parent, length, value, comp)
        if parent == 0:
            return
        parent -= 1


def _pop_heap(a, first, last, result, comp):
    value = a[result]
    a[result] = a[first]
    _adjust_heap(a, first, 0, last - first, value, comp)


def _heap_select(a, first, middle, last, comp):
    _make_heap(a, first, middle, comp)
    for i in range(middle, last):
        if comp(a[i], a[first]):
            _pop_heap(a, first, middle, i, comp)


def _sort_heap(a, first, last, comp):
    while last - first > 1:
        last -= 1
        _pop_heap(a, first, last, last, comp)


def partial_sort(a, first, middle, last, comp):
    """std::partial_sort(a + first, a + middle, a + last, comp) as libstdc++ implements it."""
    _heap_select(a, first, middle, last, comp)
    _sort_heap(a, first, middle, comp)


# ---------------------------------------------------------------- the solver's arrays, read in place
class Arrays:
    """Views of the solver's internal SoA after mcf_ns_begin (mcf_ns_internal): they follow every mcf_ns_apply_pivot."""

    def __init__(self, ns):
        ms, cap = C.c_int32(), C.c_int32()
        ps, pt = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        pc, ppi, pst = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_int8)()
        L.check(L.lib().mcf_ns_internal(ns._h, C.byref(ms), C.byref(cap), C.byref(ps), C.byref(pt), C.byref(pc), C.byref(pst), C.byref(ppi)))
        a, n1 = cap.value, ns.node_count + 1
        self.search_arc_num = ms.value
        self.source = np.ctypeslib.as_array(ps, shape=(a,))
        self.target = np.ctypeslib.as_array(pt, shape=(a,))
        self.cost = np.ctypeslib.as_array(pc, shape=(a,))
        self.state = np.ctypeslib.as_array(pst, shape=(a,))
        self.pi = np.ctypeslib.as_array(ppi, shape=(n1,))

    def c(self, e):
        return int(self.state[e]) * (int(self.cost[e]) + int(self.pi[self.source[e]]) - int(self.pi[self.target[e]]))

    def costs(self, lo, hi):
        """c of the arcs lo .. hi - 1 (ns.h:480 / :588) as int64"""
        s, t = self.source[lo:hi], self.target[lo:hi]
        return self.state[lo:hi].astype(np.int64) * (self.cost[lo:hi] + self.pi[s] - self.pi[t])


_RUN = 4096


def _eligible(ar, lo, hi):
    """(e, c) for every arc e of lo .. hi - 1 in increasing order with c < 0"""
    for a in range(lo, hi, _RUN):
        b = min(hi, a + _RUN)
        c = ar.costs(a, b)
        for i in np.flatnonzero(c < 0):
            yield a + int(i), int(c[i])


class CandidateListLiteral:
    """ns.h:415-510"""

    def __init__(self, ar):
        self.ar = ar
        self._search_arc_num = ar.search_arc_num
        self._next_arc = 0
        LIST_LENGTH_FACTOR = 0.25
        MIN_LIST_LENGTH = 10
        MINOR_LIMIT_FACTOR = 0.1
        MIN_MINOR_LIMIT = 3
        self._list_length = max(int(LIST_LENGTH_FACTOR * math.sqrt(float(self._search_arc_num))), MIN_LIST_LENGTH)
        self._minor_limit = max(int(MINOR_LIMIT_FACTOR * self._list_length), MIN_MINOR_LIMIT)
        self._curr_length = self._minor_count = 0
        self._candidates = [0] * self._list_length
        self.majors = self.minors = 0

    def findEnteringArc(self):
        """the entering arc, or None (return false)"""
        ar = self.ar
        in_arc = None
        if self._curr_length > 0 and self._minor_count < self._minor_limit:
            # Minor iteration: select the best eligible arc from the current candidate list
            self._minor_count += 1
            min_ = 0
            i = 0
            while i < self._curr_length:
                e = self._candidates[i]
                c = ar.c(e)
                if c < min_:
                    min_ = c
                    in_arc = e
                elif c >= 0:
                    self._curr_length -= 1
                    self._candidates[i] = self._candidates[self._curr_length]
                    i -= 1
                i += 1
            if min_ < 0:
                self.minors += 1
                return in_arc
        # Major iteration: build a new candidate list
        self.majors += 1
        min_ = 0
        self._curr_length = 0
        stop = None
        for lo, hi in ((self._next_arc, self._search_arc_num), (0, self._next_arc)):
            for e, c in _eligible(ar, lo, hi):
                self._candidates[self._curr_length] = e
                self._curr_length += 1
                if c < min_:
                    min_ = c
                    in_arc = e
                if self._curr_length == self._list_length:
                    stop = e                                  # goto search_end
                    break
            if stop is not None:
                break
        if stop is None:
            if self._curr_length == 0:
                return None
            stop = self._next_arc                             # e after the second loop
        self._minor_count = 1
        self._next_arc = stop
        return in_arc


class AlteringListLiteral:
    """ns.h:514-633"""

    def __init__(self, ar):
        self.ar = ar
        self._search_arc_num = ar.search_arc_num
        self._next_arc = 0
        self._cand_cost = [0] * self._search_arc_num
        BLOCK_SIZE_FACTOR = 1.0
        MIN_BLOCK_SIZE = 10
        HEAD_LENGTH_FACTOR = 0.01
        MIN_HEAD_LENGTH = 3
        self._block_size = max(int(BLOCK_SIZE_FACTOR * math.sqrt(float(self._search_arc_num))), MIN_BLOCK_SIZE)
        self._head_length = max(int(HEAD_LENGTH_FACTOR * self._block_size), MIN_HEAD_LENGTH)
        self._candidates = [0] * (self._head_length + self._block_size)
        self._curr_length = 0
        self.majors = self.minors = 0

    def _sort_func(self, left, right):
        return self._cand_cost[left] < self._cand_cost[right]

    def findEnteringArc(self):
        ar = self.ar
        # Check the current candidate list
        i = 0
        while i != self._curr_length:
            e = self._candidates[i]
            c = ar.c(e)
            if c < 0:
                self._cand_cost[e] = c
            else:
                self._curr_length -= 1
                self._candidates[i] = self._candidates[self._curr_length]
                i -= 1
            i += 1
        # Extend the list
        self.majors += 1
        cnt = self._block_size
        limit = self._head_length
        stop = None
        for lo, hi in ((self._next_arc, self._search_arc_num), (0, self._next_arc)):
            e = lo
            while e < hi:
                # the arcs up to the next block boundary (or the end of this loop), then `if (--cnt == 0)` for the last of them
                seg = min(hi, e + cnt)
                for a, c in _eligible(ar, e, seg):
                    self._cand_cost[a] = c
                    self._candidates[self._curr_length] = a
                    self._curr_length += 1
                cnt -= seg - e
                e = seg
                if cnt == 0:
                    if self._curr_length > limit:
                        stop = e - 1                          # goto search_end with e = the block's last arc
                        break
                    limit = 0
                    cnt = self._block_size
            if stop is not None:
                break
        if stop is None:
            if self._curr_length == 0:
                return None
            stop = self._next_arc
        # Perform partial sort operation on the candidate list
        new_length = min(self._head_length + 1, self._curr_length)
        partial_sort(self._candidates, 0, new_length, self._curr_length, self._sort_func)
        # Select the entering arc and remove it from the list
        in_arc = self._candidates[0]
        self._next_arc = stop
        self._candidates[0] = self._candidates[new_length - 1]
        self._curr_length = new_length - 1
        return in_arc


def solve_literal(ns, rule):
    """Solve() with the literal rule on the library's sequential half.  Returns (status, trace, rule object)."""
    st = ns.begin()
    if st != NOT_SOLVED:
        return st, np.zeros(0, np.int32), None
    ar = Arrays(ns)
    r = CandidateListLiteral(ar) if rule == CANDIDATE_LIST else AlteringListLiteral(ar)
    max_iter = max(1000000, ns.node_count * ns.arc_count)            # NS.cs:280
    trace = []
    status = NOT_SOLVED
    while True:
        arc = r.findEnteringArc()
        if arc is None:
            break
        trace.append(arc)
        if len(trace) > max_iter:                                       # NS.cs:311-317
            status = INFEASIBLE
            break
        if ns.apply_pivot(arc):
            status = UNBOUNDED
            break
    if status == NOT_SOLVED:
        status = ns.finish()
    return status, np.array(trace, np.int32), r
