"""The look-back protocol of csrc/lookback.h as a specification in plain Python, and the table of record states that takes every
branch of it on purpose (tests/test_lookback_cases_cpu.py proves that from this file alone; tests/test_gpu_lookback_protocol.py
runs the table on the device through ii2_lookback_check).

The protocol: workgroup g of a launch publishes its amount in agg[g]; the last workgroup of every group of 64 (and the launch's
last one) publishes the group's amount in grp[2 G] and, once it knows its own prefix, the amount of everything up to and
including its group in grp[2 G + 1].  A record is READY when it carries the launch's epoch, whatever else it holds.  Workgroup
g = 64 G + i finds the sum of the amounts before it like this:

  * the members of its own group before it, by their amounts;
  * all 64 members of group G - 1, by their amounts (never by that group's records);
  * then the groups from G - 2 down, in windows of 32 groups, nearest first.  In a window the nearest group whose prefix is
    ready ends the walk, once the amounts of all groups nearer than it (in that window) are ready: they and that prefix are
    added.  A window without a ready prefix whose amounts are all ready is added and the walk moves on to the next 32 groups,
    down to group 0.  Anything else is waited for - on records nobody is going to write that is a give-up.

The walk() below restates this; Rules holds the places where an implementation can go wrong in a way no fault would show,
each as a switch, so that the CPU test can show which case of the table tells the wrong rule from the right one."""
import zlib
from dataclasses import dataclass, field, replace

import numpy as np

GROUP, WINDOW = 64, 32
VALUE_BITS = 40
MASK = (1 << VALUE_BITS) - 1
EPOCH_MAX = (1 << 24) - 1
MISSING, READY, STALE, LATER = range(4)                  # II2_LB_SEED_*: all zero / this epoch / the one before / the one after
GAVE_UP_PREFIX, GAVE_UP_GROUP, NO_PREFIX = 1, 2, 0xFF    # II2_LB_GAVE_UP_*, II2_LB_NO_PREFIX
SPIN, SPIN_GIVE_UP = 4096, 64                            # polls a wait may take: every case / the cases that must give up
SIZES = (1, 2, 63, 64)                                   # launched workgroups of a seeded case (one group, whole or partial)


class Records:
    """What a launch finds in the records of the G groups before the launched one: per record a state and a raw 40-bit value.
    agg: the 64 G workgroups' amounts; amt / pre: per group its amount (grp[2 j]) and its inclusive prefix (grp[2 j + 1])."""

    def __init__(self, G):
        self.G = G
        self.state = {"agg": np.zeros(GROUP * G, np.uint8), "amt": np.zeros(G, np.uint8), "pre": np.zeros(G, np.uint8)}
        self.value = {"agg": np.zeros(GROUP * G, np.uint64), "amt": np.zeros(G, np.uint64), "pre": np.zeros(G, np.uint64)}

    def put(self, kind, i, state, value):
        assert 0 <= int(value) <= MASK
        self.state[kind][i], self.value[kind][i] = state, value

    def get(self, kind, i):
        return int(self.state[kind][i]), int(self.value[kind][i])

    def copy(self):
        r = Records(self.G)
        r.state = {k: v.copy() for k, v in self.state.items()}
        r.value = {k: v.copy() for k, v in self.value.items()}
        return r

    def keys(self):
        return [(k, i) for k in ("agg", "amt", "pre") for i in range(self.state[k].size)]

    def seeds(self):
        """(seed_state, seed_value) as ii2_lookback_check takes them: the amounts, then {amount, prefix} group by group"""
        grp_s = np.stack([self.state["amt"], self.state["pre"]], 1).reshape(-1)
        grp_v = np.stack([self.value["amt"], self.value["pre"]], 1).reshape(-1)
        return np.concatenate([self.state["agg"], grp_s]).astype(np.uint8), np.concatenate([self.value["agg"], grp_v]).astype(np.uint64)


@dataclass(frozen=True)
class Rules:
    step: int = WINDOW                # groups the walk moves on by after a window without a prefix
    part_through: bool = False        # in front of a prefix at place d: the amounts nearer than d (False), or those through d
    need_through: bool = False        # ... and the amounts that have to be ready for it: the same choice
    hi_bits: int = 0                  # 0: sums are sums; n: the values' bits above 20 are cut to n bits before a sum (lb_wave_sum64)
    ready: tuple = (READY,)           # the states that count as ready


SPEC = Rules()
# the ways of getting it wrong that the table has to tell from SPEC (one switch each)
WRONG = {
    "window step 31": replace(SPEC, step=WINDOW - 1),
    "partial sum through d": replace(SPEC, part_through=True),
    "need through d": replace(SPEC, need_through=True),
    "16-bit upper half": replace(SPEC, hi_bits=16),
    "later epoch is ready": replace(SPEC, ready=(READY, LATER)),
    "stale is ready": replace(SPEC, ready=(READY, STALE)),
}


@dataclass
class Walk:
    prefix: object                    # the sum of the amounts before the workgroup; None: it gives up
    windows: int = 0                  # windows of group records looked at
    dist: int = NO_PREFIX             # place (0 .. 31) in the last window of the prefix record that ended the walk
    read: frozenset = frozenset()     # the records whose values are in the sum: ("agg" | "amt" | "pre", index) / ("live", i)


def _sum(values, rules):
    if not rules.hi_bits:
        return sum(values)
    return sum(v & 0xFFFFF for v in values) + (sum((v >> 20) & ((1 << rules.hi_bits) - 1) for v in values) << 20)


def walk(rec, i, live, rules=SPEC):
    """Workgroup g = 64 rec.G + i of a launch whose workgroups 64 rec.G .. publish live[0], live[1], ... (always ready in the
    end) and find `rec` in everything before them."""
    G = rec.G
    ok = lambda st: st in rules.ready
    read = {("live", k) for k in range(i)}
    total = _sum([int(live[k]) for k in range(i)], rules)
    if G >= 1:
        members = [rec.get("agg", GROUP * (G - 1) + k) for k in range(GROUP)]
        if not all(ok(s) for s, _ in members):
            return Walk(None)
        total += _sum([v for _, v in members], rules)
        read |= {("agg", GROUP * (G - 1) + k) for k in range(GROUP)}
    top, windows, dist = G - 2, 0, NO_PREFIX
    while top >= 0:
        windows += 1
        groups = [top - k for k in range(WINDOW) if top - k >= 0]              # nearest first
        with_prefix = [k for k, j in enumerate(groups) if ok(rec.get("pre", j)[0])]
        if with_prefix:
            d = with_prefix[0]
            need = [j for j in groups[:d + 1 if rules.need_through else d]]
            if not all(ok(rec.get("amt", j)[0]) for j in need):
                return Walk(None, windows)
            part = groups[:d + 1 if rules.part_through else d]
            total += _sum([rec.get("amt", j)[1] for j in part], rules) + rec.get("pre", groups[d])[1]
            read |= {("amt", j) for j in part} | {("pre", groups[d])}
            dist = d
            break
        if not all(ok(rec.get("amt", j)[0]) for j in groups):
            return Walk(None, windows)
        total += _sum([rec.get("amt", j)[1] for j in groups], rules)
        read |= {("amt", j) for j in groups}
        top -= rules.step
    return Walk(total, windows, dist, frozenset(read))


# ---- the table ----------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    G: int                            # group of the launched workgroups: g_base = 64 G
    branch: str                       # what the case pins
    setup: object                     # (Records, rng) -> None: the groups 0 .. G - 2 (everything else is set before it)
    windows: int                      # what the walk must be ...
    dist: int = NO_PREFIX
    gives_up: bool = False
    live: object = None               # the 64 amounts of the launched group (None: small ones, zeros among them)
    epoch: object = None              # the epoch the case runs at (None: whatever comes next)
    last_prefix: object = None        # the prefix of the 64th launched workgroup, where the case is built around it
    pins: tuple = ()                  # names of WRONG whose result this case must change

    def rng(self):
        return np.random.default_rng(zlib.crc32(self.name.encode()))

    def records(self):
        """Everything before the launched group.  Group G - 1's amounts are ready (every walk needs them); its two group records,
        which no walk reads, and the amounts of all workgroups before it, which no walk reads either, hold ready decoys.  The
        groups 0 .. G - 2 start with ready amounts and no prefix; `setup` then makes the case."""
        rng, rec, G = self.rng(), Records(self.G), self.G
        for g in range(GROUP * G):
            rec.put("agg", g, READY, int(rng.integers(1, 1 << 20)))
        if G >= 1:
            rec.put("amt", G - 1, READY, int(rng.integers(1 << 24, 1 << 25)))
            rec.put("pre", G - 1, READY, int(rng.integers(1 << 34, 1 << 35)))
        for j in range(G - 1):
            rec.put("amt", j, READY, int(rng.integers(1, 1 << 24)))
        self.setup(rec, rng)
        return rec

    def amounts(self):
        if self.live is not None:
            return np.array(self.live, np.uint64)
        a = self.rng().integers(1, 1000, GROUP).astype(np.uint64)
        a[[0, 5, 62]] = 0
        return a


def _prefix_value(rng):
    return int(rng.integers(1 << 30, 1 << 34))            # (some below 2^32, some above)


def _nothing(rec, rng):
    pass


def _prefix_at(top, d, far_ready=True):
    """a ready prefix at place d of the window that starts at group `top`; the amount of that same group is stale and not
    zero (it is neither needed nor added); behind it ready prefixes and unready amounts that must not be used"""
    def setup(rec, rng):
        j = top - d
        rec.put("pre", j, READY, _prefix_value(rng))
        rec.put("amt", j, STALE, int(rng.integers(1, 1 << 24)))
        for f in range(j):
            rec.put("pre", f, READY if far_ready else MISSING, _prefix_value(rng))
            rec.put("amt", f, (MISSING, STALE, LATER)[f % 3], int(rng.integers(1, 1 << 24)))
    return setup


def _unready_prefixes(rec, rng):
    """no ready prefix anywhere, but prefix records that are NOT ready in every other group (stale, later, stale, ...)"""
    for j in range(0, rec.G - 1, 2):
        rec.put("pre", j, (STALE, LATER)[(j // 2) % 2], _prefix_value(rng))


def _nearer_unready(state):
    def setup(rec, rng):
        top = rec.G - 2
        _prefix_at(top, 9)(rec, rng)
        rec.put("pre", top - 3, state, _prefix_value(rng))
    return setup


def _unready_amount_before_prefix(state):
    def setup(rec, rng):
        top = rec.G - 2
        _prefix_at(top, 6)(rec, rng)
        rec.put("amt", top - 2, state, int(rng.integers(1, 1 << 24)))
    return setup


def _missing_amount_no_prefix(rec, rng):
    _unready_prefixes(rec, rng)
    rec.put("amt", 20, MISSING, 0)


# 40-bit arithmetic: values at and above 2^32 and around 2^39 in every kind of record, and the 64th launched workgroup's prefix
# exactly 2^40 - 1: what is still missing to that goes into one amount of group G - 1
BIG_LIVE = [0] * GROUP
BIG_LIVE[0], BIG_LIVE[1], BIG_LIVE[40] = (1 << 36) + 0xABCDE, (1 << 32), (1 << 37) + (1 << 20) + 7


def _big(with_prefix):
    def setup(rec, rng):
        G, top = rec.G, rec.G - 2
        for j in range(G - 1):
            rec.put("amt", j, READY, int(rng.integers(0, 1 << 12)))
        if with_prefix:
            _prefix_at(top, 2)(rec, rng)
            rec.put("pre", top - 2, READY, (1 << 39) + 0x12345678)         # (both halves of the 64-bit read carry bits)
            rec.put("amt", top, READY, (1 << 36) + (1 << 35) + 0xFFFFF)
            rec.put("amt", top - 1, READY, (1 << 32) + 1)
        else:
            rec.put("amt", top, READY, (1 << 38) + 0xFFFFF)                # one in every window
            rec.put("amt", top - WINDOW - 3, READY, (1 << 37) + (1 << 36) + 5)
            rec.put("amt", 1, READY, (1 << 36) + (1 << 33))
            _unready_prefixes(rec, rng)
        for k in range(GROUP):
            rec.put("agg", GROUP * (G - 1) + k, READY, int(rng.integers(0, 1 << 12)))
        rec.put("agg", GROUP * (G - 1) + 63, READY, (1 << 37) + (1 << 21))
        rec.put("agg", GROUP * (G - 1) + 17, READY, 0)
        rest = MASK - walk(rec, GROUP - 1, BIG_LIVE).prefix
        assert (1 << 32) <= rest <= MASK
        rec.put("agg", GROUP * (G - 1) + 17, READY, rest)
    return setup


def _all_ones(rec, rng):
    """at the last epoch before the wrap a ready record holding 2^40 - 1 is 64 one-bits; everything else it is added to is zero"""
    G = rec.G
    for k in range(GROUP):
        rec.put("agg", GROUP * (G - 1) + k, READY, 0)
    _prefix_at(G - 2, 0)(rec, rng)
    rec.put("pre", G - 2, READY, MASK)


CASES = [
    Case("g0", 0, "no group before: nothing but the own group's members", _nothing, 0),
    Case("g1", 1, "one group before: its members, no window", _nothing, 0),
    Case("g2", 2, "the smallest window (group 0 alone), left by its amount", _nothing, 1),
    Case("g2_prefix_d0", 2, "prefix at distance 0", _prefix_at(0, 0), 1, 0, pins=("partial sum through d", "need through d")),
    Case("g33_prefix_d0", 33, "prefix at distance 0", _prefix_at(31, 0), 1, 0, pins=("partial sum through d", "need through d")),
    Case("g33_prefix_d31", 33, "prefix in the last lane of the window", _prefix_at(31, 31), 1, 31, pins=("partial sum through d", "need through d")),
    Case("g33_no_prefix", 33, "one whole window without a prefix, then top < 0", _unready_prefixes, 1, pins=("later epoch is ready", "stale is ready")),
    Case("g34_no_prefix", 34, "the window is left; group 0 alone makes the second", _unready_prefixes, 2, pins=("window step 31",)),
    Case("g35_no_prefix", 35, "two windows, then the end", _unready_prefixes, 2, pins=("window step 31",)),
    Case("g66_no_prefix", 66, "three windows (the last: group 0), then the end", _unready_prefixes, 3, pins=("window step 31",)),
    Case("g67_no_prefix", 67, "three windows, then the end", _unready_prefixes, 3, pins=("window step 31",)),
    Case("g70_later_window_d0", 70, "prefix found in the second window, at 0", _prefix_at(36, 0), 2, 0, pins=("window step 31", "need through d")),
    Case("g70_later_window_d5", 70, "prefix found in the second window, at 5", _prefix_at(36, 5), 2, 5, pins=("window step 31", "partial sum through d")),
    Case("g70_later_window_d31", 70, "prefix found in the second window, in its last lane", _prefix_at(36, 31), 2, 31, pins=("window step 31",)),
    Case("g40_stale_prefix", 40, "a nearer prefix of the epoch before is not ready", _nearer_unready(STALE), 1, 9, pins=("stale is ready",)),
    Case("g40_later_prefix", 40, "a nearer prefix of a later epoch is not ready", _nearer_unready(LATER), 1, 9, pins=("later epoch is ready",)),
    Case("g40_stale_amount", 40, "a stale amount in front of a ready prefix: give-up", _unready_amount_before_prefix(STALE), 1, gives_up=True,
         pins=("stale is ready",)),
    Case("g40_later_amount", 40, "an amount of a later epoch in front of a ready prefix: give-up", _unready_amount_before_prefix(LATER), 1,
         gives_up=True, pins=("later epoch is ready",)),
    Case("g40_missing_amount", 40, "an amount missing in a window without a prefix: give-up", _missing_amount_no_prefix, 1, gives_up=True),
    Case("g40_big", 40, "40-bit values: prefix above 2^39, amounts above 2^32, the result 2^40 - 1", _big(True), 1, 2, live=BIG_LIVE,
         last_prefix=MASK, pins=("16-bit upper half",)),
    Case("g70_big", 70, "40-bit values through three windows of amounts, the result 2^40 - 1", _big(False), 3, live=BIG_LIVE,
         last_prefix=MASK, pins=("16-bit upper half", "window step 31")),
    Case("g70_all_ones", 70, "value 2^40 - 1 at epoch 2^24 - 1: a record of 64 one-bits", _all_ones, 1, 0, live=[0] * GROUP, epoch=EPOCH_MAX,
         last_prefix=MASK),
    Case("g80_all_ones", 80, "value 2^40 - 1 at epoch 2^24 - 1: a record of 64 one-bits", _all_ones, 1, 0, live=[0] * GROUP, epoch=EPOCH_MAX,
         last_prefix=MASK),
]
BY_NAME = {c.name: c for c in CASES}


def expected_records(case, k, epoch):
    """The raw records of the launched group after a run of k workgroups that did not give up: (agg [k], {amount, prefix})"""
    live = case.amounts()[:k]
    tag = epoch << VALUE_BITS
    first = walk(case.records(), 0, live).prefix
    total = int(live.sum())
    return [tag | int(a) for a in live], [tag | (total & MASK), tag | ((first + total) & MASK)]


# ---- live grids: every workgroup launched, nothing seeded -----------------------------------------------------------------------
LIVE_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 2112, 2176, 2177, 4096, 4097, 100_000)
LIVE_DELAY_EVERY, LIVE_DELAY = 7, 64          # every 7th workgroup publishes 64 units late: 1/64 of what SPIN polls wait for


def live_amounts(n_wg, seed=0):
    """amounts with zeros and a few huge values among them; the sum stays below 2^40"""
    rng = np.random.default_rng(1000 + n_wg + seed)
    a = rng.integers(0, 5000, n_wg).astype(np.uint64)
    a[rng.random(n_wg) < 0.2] = 0
    huge = [(1 << 38) + 0xFEDCB, (1 << 37) + (1 << 36) + 1, (1 << 36) + (1 << 20), (1 << 32) + 3, (1 << 32) - 1]
    for h, at in zip(huge, rng.choice(n_wg, min(len(huge), n_wg), replace=False)):
        a[at] = h
    assert int(a.sum()) <= MASK
    return a


def live_delays(n_wg):
    d = np.zeros(n_wg, np.uint16)
    d[LIVE_DELAY_EVERY - 1::LIVE_DELAY_EVERY] = LIVE_DELAY
    return d


def live_expected(amounts, epoch):
    """(prefix per workgroup, raw agg records, raw grp records) of a launch of all of them"""
    a = amounts.astype(np.uint64)
    incl = np.cumsum(a, dtype=np.uint64)
    tag = np.uint64(epoch << VALUE_BITS)
    n_grp = (a.size + GROUP - 1) // GROUP
    ends = np.minimum(np.arange(1, n_grp + 1) * GROUP, a.size) - 1
    grp_incl = incl[ends]
    grp_sum = np.diff(np.concatenate([[np.uint64(0)], grp_incl]).astype(np.uint64))
    return incl - a, tag | a, np.stack([tag | grp_sum, tag | grp_incl], 1).reshape(-1)
