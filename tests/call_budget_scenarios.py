"""Scenarios around the 64-call budget of nested mixers (PG_MAX_CALLS, pg_dev.h): a parent mixer P whose events cut one chunk of the main mixer
into 63 / 64 / 65 / 130 calls of its child C, with the reference's per-call decisions — C's silence gate (submixer.rs:47-77) and the bypass
of P's effect chain (mixed/effect.rs:56-145) — placed at chosen calls of that chunk. Shared by tests/test_call_budget_scenarios.py (the CPU
pre-check against the oracle) and tests/test_gpu_call_budget.py.

Topology, at 8000 Hz (the gate is SILENCE_SECONDS * sample_rate = 16000 frames):

    main [-> Gain -> Delay] <- P (own one-shot voice; Gain -> Delay) <- C (one-shot voice; Gain)
                            <- Q (the same, optional)               <- D

C has no effect with a tail: it is exactly silent behind its voice's last frame, and P takes an event at frame S right behind it, so the gate
counts the frames of P's calls from S on and expires in the call that holds frame S + 15999. The one-shot's length moves S and with it that call.
From there the chain of P runs down call by call (`chain_onset`): Gain bypasses one call later, the Delay takes its tail from the call after that
and is bypassed once the calls behind it add up to the tail — P's output trickles until then and is exactly zero from that call's first frame
on. A decision that moves by one call moves that frame; the samples in between are far below every parity tolerance."""
import numpy as np

from phonic_amd import _capi, workloads

SR = 8000
BLOCK = 1024
CHUNK = 4096                         # MixedSource::MAX_MIX_BUFFER_SAMPLES / 2
BUDGET = 64                          # PG_MAX_CALLS
GATE = 2 * SR                        # SILENCE_SECONDS * sample_rate
USIZE_MAX = 2**64 - 1
P_DELAY = {"dlay": 30.0, "fdbk": 0.3, "wet_": 0.6}     # (test_deferred_bus_words_follow_the_pieces_when_events_cut_the_call)
MAIN_DELAY = {"dlay": 60.0, "fdbk": 0.3, "wet_": 0.6}  # (a longer period: the main bus still trickles in normal f32 numbers when its chain bypasses)
GAIN = {"gain": 0.8}


def spacings(n, room):
    """n odd spacings of 7..29 frames, cycling through as wide a set as fits `room` frames."""
    for cyc in ([23, 25, 27, 29], [9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29], [7, 9, 11, 13, 15, 17, 19, 21], [7, 9, 11, 13, 15], [7, 9, 11], [7, 7, 9]):
        s = [cyc[i % len(cyc)] for i in range(n)]
        if sum(s) <= room:
            return s
    raise ValueError((n, room))


class Scenario:
    """n_cuts distinct event times inside every dense chunk; `place`: the call of the target chunk (0-based, call j begins at cut j - 1) in which
    C's gate expires. call_frames: frames per write call (1024, or 4096: the chunk is four pieces of 1024 / sixteen of 256)."""

    def __init__(self, name, n_cuts, place, max_frames=1024, call_frames=BLOCK, two_parents=False, main_chain=False):
        self.name, self.n_cuts, self.place, self.max_frames, self.call_frames = name, n_cuts, place, max_frames, call_frames
        self.two_parents, self.main_chain = two_parents, main_chain
        L = call_frames
        self.offsets = list(np.cumsum(spacings(n_cuts, L - 8)))
        assert len(set(self.offsets)) == n_cuts and 0 < self.offsets[0] and self.offsets[-1] < L
        # the target chunk T, an early chunk with the same cuts while the voices play, and the chunks behind T up to where P's chain has run down:
        # those are cut every 7 frames (the shortest spacing), so that a decision of T that moves by one call moves the chain's last call too
        if call_frames == BLOCK:
            self.target = 17 if main_chain else 18
            self.dense, self.follow = [1, self.target], [] if main_chain else list(range(self.target + 1, self.target + 7))
            self.n_calls = 28
        else:
            self.target = 4
            self.dense, self.follow = [0, 4], [] if main_chain else [5]
            self.n_calls = 10 if main_chain else 7
        # (with 4096-frame calls the main chain runs down over 8 chunks: a longer period keeps its trickle in normal f32 numbers until then)
        self.main_delay = MAIN_DELAY if call_frames == BLOCK else dict(MAIN_DELAY, dlay=100.0)
        self.fine = list(range(7, min(L - 8, 2400), 7))
        self.t0 = self.target * L
        # who owns cut i: with two parents every third cut is Q's (never the cuts at which the budget ends a chunk: 63, 127)
        self.owner = ["Q" if (two_parents and i % 3 == 1) else "P" for i in range(n_cuts)]
        assert place >= 1 and self.owner[place - 1] == "P"
        lo = self.t0 + self.offsets[place - 1]
        own_after = [self.t0 + o for i, o in enumerate(self.offsets) if i >= place and self.owner[i] == "P"] + [self.t0 + L]
        self.expiry_call = (lo, own_after[0])
        x = lo + (own_after[0] - lo) // 2                     # the frame at which the gate's count reaches 16000
        self.s_p = x - (GATE - 1)                              # P's event right behind C's last frame
        self.c_len = self.s_p - 5
        # P's own voice: ends some hundred frames in front of the gate's expiry, so that the chain still rings audibly when its input flag drops;
        # with a main chain it ends early instead (frame 1034): then P is below the threshold for the main mixer's gate from the chunk behind
        # its echoes on — chunk 2 of 1024 frames, chunk 1 of 4096 — and that gate expires in T too
        self.p_len = BLOCK + 10 if main_chain else lo - 700
        if main_chain:                                         # (C ends with P's voice: its gate is not this scenario's subject)
            self.c_len = self.p_len - 20
            self.s_p = self.c_len + 5
        self.s_q = self.s_p + 41
        self.d_len = self.s_q - 5
        self.q_len = self.p_len - 100
        assert self.c_len > 16 and self.p_len > 16
        self.total = self.n_calls * L
        self.events = self._events()

    # ---- events: (time, mixer, kind, value) -----------------------------------------------------------------------------------------
    def _events(self):
        ev = []
        for c in self.dense + self.follow:
            base = c * self.call_frames
            for i, o in enumerate(self.offsets if c in self.dense else self.fine):
                t = base + int(o)
                who = self.owner[i % self.n_cuts]
                alive = t + 64 < (self.p_len if who == "P" else self.q_len)
                kind = ("gain", "volume", "gain", "panning")[i % 4] if alive else "gain"
                val = {"gain": 0.8 + 0.01 * (i % 5), "volume": 0.5 - 0.02 * (i % 3), "panning": 0.1 * ((i % 5) - 2)}[kind]
                ev.append((t, who, kind, val))
                if i % 9 == 4:                                 # duplicate times: a second event of the same mixer — of the other parent, if there is one
                    ev.append((t, ("Q" if who == "P" else "P") if self.two_parents else who, "gain", 0.8 + 0.01 * ((i + 2) % 5)))
        ev.append((self.s_p, "P", "gain", 0.83))
        if self.two_parents:
            ev.append((self.s_q, "Q", "gain", 0.84))
        return sorted(ev, key=lambda e: e[0])

    def cuts(self, mixer=None):
        """Sorted distinct event times (of one parent, or of all)."""
        return sorted(set(t for t, who, _, _ in self.events if mixer is None or who == mixer))

    def cuts_in_chunk(self, start, mixer=None):
        return [t for t in self.cuts(mixer) if start < t < start + self.call_frames]

    def grid(self, mixer):
        """Boundaries of the write calls that the parent `mixer` makes to its child: the main mixer's chunks and the parent's own events."""
        b = set(range(0, self.total + 1, self.call_frames)) | set(t for t in self.cuts(mixer) if t < self.total)
        return sorted(b)

    # ---- building and rendering -----------------------------------------------------------------------------------------------------
    def build(self, g, solo=None, main_chain=None):
        """-> ids. solo = "C": P without voice, effects and events, so that the bus is C's output alone (the metering test's reference).
        main_chain = False: leave the main mixer's chain out (the bus is then what the main mixer's gate sees of P)."""
        ids = {}
        if (self.main_chain if main_chain is None else main_chain) and solo is None:
            ids["main_gain"] = g.add_effect(0, _capi.FX_GAIN, params=GAIN)
            ids["main_delay"] = g.add_effect(0, _capi.FX_DELAY, params=self.main_delay)
        for k, (par, child, plen, clen) in enumerate((("P", "C", self.p_len, self.c_len), ("Q", "D", self.q_len, self.d_len))[: 2 if self.two_parents and solo is None else 1]):
            m = g.add_mixer()
            ids[par] = m
            if solo is None:
                ids[par + "_gain"] = g.add_effect(m, _capi.FX_GAIN, params=GAIN)
                ids[par + "_delay"] = g.add_effect(m, _capi.FX_DELAY, params=P_DELAY)
                ids[par + "_voice"] = g.add_voice(m, workloads.tone_buffer(3 + 10 * k, SR, plen / SR), 2, SR, volume=0.5, panning=0.1 if k else -0.1)
            c = g.add_mixer(m)
            ids[child] = c
            g.add_effect(c, _capi.FX_GAIN, params={"gain": 0.9})
            g.add_voice(c, workloads.tone_buffer(7 + 10 * k, SR, clen / SR), 2, SR, volume=0.5)
        return ids

    def schedule(self, g, ids, lo, hi):
        """The events with lo <= time < hi, as the caller of a write call [lo, hi) schedules them in front of it. -> how many."""
        n = 0
        for t, who, kind, val in self.events:
            if not lo <= t < hi:
                continue
            if kind == "gain":
                g.schedule_param(ids[who + "_gain"], "gain", val, t)
            elif kind == "volume":
                g.set_voice_volume(ids[who + "_voice"], val, t)
            else:
                g.set_voice_panning(ids[who + "_voice"], val, t)
            n += 1
        return n

    def render(self, g, solo=None, n_calls=None, main_chain=None):
        ids = self.build(g, solo, main_chain)
        L = self.call_frames
        n_calls = n_calls or self.n_calls
        out = np.zeros((n_calls, 2 * L), np.float32)
        for b in range(n_calls):
            if solo is None:
                self.schedule(g, ids, b * L, (b + 1) * L)
            w = g.write(out[b], b * L)
            assert w in (0, 2 * L), w
        return out.reshape(-1)


# ---- the reference's decisions, restated ---------------------------------------------------------------------------------------------------
def gate_expiry(grid, first_silent):
    """Index i of the call [grid[i], grid[i + 1]) in which a SubMixerProcessor's silence count, started with the call at grid[i] == first_silent,
    reaches the gate: that call and every later one returns false."""
    i = grid.index(first_silent)
    count = 0
    while True:
        count += grid[i + 1] - grid[i]
        if count >= GATE:
            return i
        i += 1


def chain_onset(grid, k, tails):
    """EffectProcessor::process for every effect of a chain (tails: Effect::process_tail of each, in frames) over the calls of `grid` from call k on,
    the first whose input flag is off; before it the chain ran with audible input. -> the first frame of the first call that the whole chain
    bypasses: with the input gone too, the mixer's output is exactly zero from there."""
    st = [dict(byp=False, tail=USIZE_MAX, sil=0) for _ in tails]
    i = k
    while i + 1 < len(grid):
        n = grid[i + 1] - grid[i]
        ib, all_byp = True, True
        for e, tf in zip(st, tails):
            should = ib and e["tail"] == 0 and e["sil"] == USIZE_MAX
            if should and not e["byp"]:
                e["byp"] = True
            elif not should and e["byp"]:
                e["byp"], e["tail"], e["sil"] = False, USIZE_MAX, 0
            if not e["byp"]:
                if ib:
                    e["tail"] = tf if e["tail"] == USIZE_MAX else max(e["tail"] - n, 0)
                    e["sil"] = USIZE_MAX
                else:
                    e["tail"], e["sil"] = USIZE_MAX, 0
                ib, all_byp = False, False
        if all_byp:
            return grid[i]
        i += 1
    raise AssertionError("the chain does not run down inside the render")


def zero_onset(bus):
    """First frame from which the interleaved stereo bus is exactly zero to its end."""
    nz = np.nonzero(bus.reshape(-1, 2).any(axis=1))[0]
    return int(nz[-1]) + 1 if nz.size else 0


def S(*a, **k):
    return Scenario(*a, **k)


# place: call 1, 62 and 63 of the chunk (bits 1, 62, 63 of the device's word), 64 / 128: the first call behind the first / second budget cut
SCENARIOS = [
    S("c63_call63", 63, 63),
    S("c63_call1_mf256", 63, 1, max_frames=256),
    S("c64_call1", 64, 1),
    S("c64_call62_mf256", 64, 62, max_frames=256),
    S("c64_call63", 64, 63),
    S("c64_restart", 64, 64),
    S("c65_call63_mf256", 65, 63, max_frames=256),
    S("c65_restart", 65, 64),
    S("c130_call63", 130, 63),
    S("c130_restart_mf256", 130, 64, max_frames=256),
    S("c130_restart2", 130, 128),
    S("c64_two_parents_restart", 64, 64, two_parents=True),
    S("c130_two_parents_call63_mf256", 130, 63, max_frames=256, two_parents=True),
    S("c64_call4096_call1", 64, 1, call_frames=4096),
    S("c130_call4096_restart_mf256", 130, 64, max_frames=256, call_frames=4096),
    S("c130_call4096_call62", 130, 62, call_frames=4096),
]
MAIN_CHAIN_SCENARIOS = [
    S("c64_main_chain", 64, 64, main_chain=True),
    S("c130_main_chain_mf256", 130, 63, max_frames=256, main_chain=True),
    S("c64_two_parents_main_chain_mf256", 64, 64, max_frames=256, two_parents=True, main_chain=True),
    S("c130_two_parents_main_chain", 130, 63, two_parents=True, main_chain=True),
    S("c130_call4096_main_chain_mf256", 130, 64, max_frames=256, call_frames=4096, main_chain=True),
]
METER_SCENARIO = S("meter70", 70, 63)   # (block 1 holds 70 events of P while C plays)
BY_NAME = {s.name: s for s in SCENARIOS + MAIN_CHAIN_SCENARIOS}
