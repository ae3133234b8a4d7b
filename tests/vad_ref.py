"""NumPy statement of the voice-activity rule (include/mimi_hip.h, mimi_vad_pool_*): per 10 ms frame a DC-free power, a first-crossing
autocorrelation lag on block-floating search samples, and a serial scan -- loud against a slow noise floor with hysteresis, voiced within
``hold`` frames, ``min_on`` active frames to start a turn, ``hang`` quiet frames to end it.  Every decision is integer arithmetic (Python
integers in the scan), so the device is held to this bit for bit.  ``vad_ref`` is the whole-clip rule; ``StreamRef`` restates it the way
the pool keeps a stream -- a carry of at most 879 samples, {N, state, run, quiet, since_voiced}, positions relative to the carry's base.
``pick='argmax'`` and ``shift=6`` are the two ways of getting the features wrong that tests/test_vad_oracle.py shows to matter."""
from collections import namedtuple

import numpy as np

F = 240                     # frame
W = 480                     # analysis window
TMIN, TMAX = 60, 400        # lags
HIST = W + TMAX - F         # samples in front of its next frame that a stream keeps: 640
CARRY = HIST + F            # int16 values a stream keeps between calls, at most CARRY - 1 = 879
SAT = 1 << 20               # since_voiced saturates here (above every legal hold)

Params = namedtuple("Params", "on_q4 off_q4 min_on hang hold n_min", defaults=(128, 48, 8, 70, 30, 3686400))


def check(p):
    ok = (p.off_q4 <= p.on_q4 <= 4095 and 16 <= p.off_q4 and 1 <= p.min_on <= 1000 and 1 <= p.hang <= 10000 and 0 <= p.hold <= 10000
          and 1 <= p.n_min <= 2 ** 40)
    if not ok:
        raise ValueError(f"parameters outside their ranges: {p}")
    return p


def to_s(x):
    """The rule's integer samples, int64: fp32 -> clamp(rint(x * 32768), -32768, 32767), a non-finite sample gives 0; int16 as it is."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.int64)
    x = x.astype(np.float32)
    with np.errstate(all="ignore"):
        v = np.clip(np.rint(x * np.float32(32768.0)), -32768.0, 32767.0)
    return np.where(np.isfinite(x), v, 0.0).astype(np.int64)


def _ext(v, lo, n):
    """v zero-extended, [lo, lo + n)"""
    out = np.zeros(n, dtype=v.dtype)
    a, b = max(lo, 0), min(lo + n, v.shape[0])
    if b > a:
        out[a - lo:b - lo] = v[a:b]
    return out


def power(fr):
    """P = F * sum(s^2) - (sum s)^2 over one frame, a Python integer"""
    s1, s2 = int(fr.sum()), int((fr * fr).sum())
    return F * s2 - s1 * s1


def correlations(buf, shift="block"):
    """buf: the W + TMAX samples that end with the frame -> (R, E, E0), R and E int64 arrays indexed by tau - TMIN."""
    m = int(np.abs(buf).max())
    sh = max(0, m.bit_length() - 10) if shift == "block" else int(shift)
    q = buf >> sh                                              # arithmetic
    w = q[TMAX:]
    qf, wf = q.astype(np.float64), w.astype(np.float64)        # (every sum is below 2^29: exact in float64 in any order)
    R = np.correlate(qf, wf, mode="valid")                     # [e] = sum_j q[e + j] w[j], e = TMAX - tau
    c = np.concatenate([[0.0], np.cumsum(qf * qf)])
    E = c[W:] - c[:TMAX + 1]                                   # [e] = sum_j q[e + j]^2
    e = TMAX - np.arange(TMIN, TMAX + 1)
    return R[e].astype(np.int64), E[e].astype(np.int64), int(E[TMAX])


def lag_of(buf, shift="block", pick="first", want_bounds=False):
    R, E, E0 = correlations(buf, shift)
    ok = [i for i in range(R.shape[0]) if int(R[i]) > 0 and 2 * int(R[i]) ** 2 > E0 * int(E[i])]
    if pick == "first":
        lag = TMIN + ok[0] if ok else 0
    else:                                                      # the best normalised correlation among those that qualify
        lag = TMIN + max(ok, key=lambda i: (int(R[i]) ** 2 / max(int(E[i]), 1), -i)) if ok else 0
    if want_bounds:
        return lag, max(2 * int(R.max()) ** 2, E0 * int(E.max()))
    return lag


def features(s, k, shift="block", pick="first"):
    """frame k of the integer samples s -> (P_k, lag_k)"""
    buf = _ext(s, (k + 1) * F - W - TMAX, W + TMAX)
    return power(buf[-F:]), lag_of(buf, shift, pick)


class Scan:
    """Steps 6 to 9: the serial part, in Python integers."""

    def __init__(self, prm):
        self.prm = check(prm)
        self.fresh()

    def fresh(self):
        self.N, self.speech, self.run, self.quiet, self.since = 0, 0, 0, 0, SAT
        self.k, self.last_start, self.last_end, self.n_start, self.n_end = 0, -1, -1, 0, 0

    def step(self, P, lag):
        """-> (flags, floor after the update, event or None)"""
        p = self.prm
        voiced = lag != 0
        if self.k == 0:
            self.N = max(P, p.n_min)
            loud = False
        else:
            loud = 16 * P > self.N * (p.off_q4 if self.speech else p.on_q4)
        self.since = 0 if voiced else min(self.since + 1, SAT)
        active = loud and self.since <= p.hold
        ev = None
        if not self.speech:
            self.run = self.run + 1 if active else 0
            if self.run == p.min_on:
                self.speech, self.run, self.quiet = 1, 0, 0
                self.last_start, self.n_start = self.k - p.min_on + 1, self.n_start + 1
                ev = ("start", self.last_start)
        else:
            self.quiet = 0 if active else self.quiet + 1
            if self.quiet == p.hang:
                self.speech, self.quiet = 0, 0
                self.last_end, self.n_end = self.k - p.hang + 1, self.n_end + 1
                ev = ("end", self.last_end)
        if P < self.N:
            self.N -= (self.N - P) >> 2
        else:
            self.N += (self.N >> 9) + 1
        self.N = max(self.N, p.n_min)
        assert 0 <= self.N < 2 ** 63 and 16 * P < 2 ** 63 and self.N * 4095 < 2 ** 63
        self.k += 1
        return int(loud) | int(voiced) << 1 | int(active) << 2 | self.speech << 3, self.N, ev

    def summary(self):
        """what mimi_vad_pool_summary holds for the stream: 8 int64"""
        return np.array([self.speech, self.k, self.last_start, self.last_end, self.quiet, self.n_start, self.n_end, 0], dtype=np.int64)


Result = namedtuple("Result", "flags lag power floor summary events")


def _pack(rows, scan, evs):
    fl, lg, pw, fo = ([r[i] for r in rows] for i in range(4))
    return Result(np.array(fl, dtype=np.uint8), np.array(lg, dtype=np.int16), np.array(pw, dtype=np.int64), np.array(fo, dtype=np.int64),
                  scan.summary(), evs)


def vad_ref(x, prm=Params(), shift="block", pick="first"):
    """x (N,) fp32 or int16 -> Result over its N // F frames; events: [("start" | "end", frame)]"""
    s = to_s(x)
    scan = Scan(prm)
    rows, evs = [], []
    for k in range(s.shape[0] // F):
        P, lag = features(s, k, shift, pick)
        flags, floor, ev = scan.step(P, lag)
        rows.append((flags, lag, P, floor))
        if ev:
            evs.append(ev)
    return _pack(rows, scan, evs)


def events(flags, prm=Params(), first=0, in_speech=False):
    """The events that a run of per-frame flags holds (bit 3 is the state after the frame): a START is stamped min_on - 1 frames before the
    frame that turns the state to speech, an END hang - 1 frames before the one that turns it back.  first: the run's first frame."""
    out, was = [], bool(in_speech)
    for i, f in enumerate(np.asarray(flags).tolist()):
        now = bool(f & 8)
        if now != was:
            out.append(("start", first + i - prm.min_on + 1) if now else ("end", first + i - prm.hang + 1))
        was = now
    return out


class StreamRef:
    """One stream the way the pool keeps it.  The carry is the integer samples from k F - HIST on (k: the next unjudged frame), in front of
    the clip's first sample nothing: positions are relative to the carry's base, the counts R and k stay with the 'host'."""

    def __init__(self, prm=Params()):
        self.reset(prm)

    def reset(self, prm):
        self.scan = Scan(prm)
        self.R, self.carry = 0, np.zeros(0, dtype=np.int64)

    def feed(self, chunk, final=False):
        k0 = self.scan.k
        base = k0 * F - HIST                                   # the absolute position of carry[0], were the carry full
        lead = max(0, -base)                                   # positions in front of the clip: zero by rule, not kept
        buf = np.concatenate([np.zeros(lead, dtype=np.int64), self.carry, to_s(chunk)])      # buf[p] = sample base + p
        assert buf.shape[0] == self.R + np.asarray(chunk).shape[0] - base
        R1 = self.R + np.asarray(chunk).shape[0]
        nf = R1 // F - k0
        rows, evs = [], []
        for i in range(nf):
            w = buf[i * F:i * F + W + TMAX]
            P, lag = power(w[-F:]), lag_of(w)
            flags, floor, ev = self.scan.step(P, lag)
            rows.append((flags, lag, P, floor))
            if ev:
                evs.append(ev)
        out = _pack(rows, self.scan, evs)
        if final:
            self.scan.fresh()
            self.R, self.carry = 0, buf[:0]
        else:
            keep = max(nf * F, lead)                           # the new base is base + nf F; what lies in front of the clip is still not kept
            self.carry, self.R = buf[keep:].copy(), R1
            assert self.carry.shape[0] < CARRY and self.carry.shape[0] == min(R1, HIST + R1 % F)
        return out


def cut(N, schedule):
    """Chunk bounds of a clip of N samples: the schedule's lengths while they fit; what is left (maybe nothing) goes with final."""
    out, at = [], 0
    for m in schedule:
        m = min(m, N - at)
        out.append((at, at + m))
        at += m
    return out, at


def vad_streamed(x, prm, schedule):
    s = StreamRef(prm)
    parts, at = cut(np.asarray(x).shape[0], schedule)
    rs = [s.feed(x[lo:hi]) for lo, hi in parts] + [s.feed(x[at:], final=True)]
    return Result(*(np.concatenate([getattr(r, f) for r in rs]) for f in ("flags", "lag", "power", "floor")), rs[-1].summary,
                  [e for r in rs for e in r.events])
