"""NumPy model of ofs_zc_detect_chunk (csrc/zc_chunk.hip): the zc_v2 CFAR + gate with its state carried
between calls.  NumPy only; it is the expected value of the GPU tests' per-call outputs (the oracle gives
the whole-stream ones) and is itself checked against ofdm_oracle in tests/test_zc_chunk_model.py.

State of one stream, exactly what the C ABI's header lists: the float64 running sum acc, the last W
magnitudes (a ring indexed by the absolute sample, zeros on a fresh stream), the sample count, and the
gate machine (open, gate_start, peak_index, peak_value, low counter).  Every step is the reference's
sample-by-sample statement (zc_v2.py:219-238, :300-346, :374-446 as restated in ofdm_oracle).
"""
import numpy as np


class ZCChunkModel:
    def __init__(self, params, hysteresis, reference_length):
        W, tv, f, mn = params
        self.W = max(1, int(W))
        self.tv, self.scale, self.mn = float(tv), float(1 << int(f)), float(mn)
        self.hyst, self.reflen = int(hysteresis), int(reference_length)
        self.reset()

    def reset(self):
        self.acc = 0.0
        self.ring = np.zeros(self.W)
        self.n = 0
        self.open = False
        self.gs = self.pk = self.low = 0
        self.pv = 0.0

    def state_arrays(self):
        """The five carried quantities of the issue's model check, as comparable values."""
        return (self.acc, self.ring.copy(), self.n, (self.open, self.gs, self.pk, self.pv), self.low)

    def _event(self, end):
        return (self.pk, self.gs, end, max(0, self.pk - self.reflen + 1))

    def push(self, c, final=False):
        """One call: dict of the chunk's arrays, its events (absolute), open_gate_start, n_events."""
        c = np.asarray(c, np.float64)
        Tc, W = c.size, self.W
        n0 = self.n
        local = np.zeros(Tc)
        valid = np.zeros(Tc, bool)
        above = np.zeros(Tc, bool)
        mask = np.zeros(Tc, bool)
        evs, vals = [], []
        lim = max(0, self.hyst - 1)
        for i in range(Tc):
            n = n0 + i
            v = c[i]
            if n >= W:
                self.acc = self.acc + v - self.ring[n % W]
                valid[i] = True
            else:
                self.acc = self.acc + v
            self.ring[n % W] = v
            local[i] = self.acc
            above[i] = valid[i] and (v * self.scale >= self.acc * self.tv) and (v >= self.mn)
            if not valid[i]:
                continue
            if not self.open:
                if above[i]:
                    self.open, self.gs, self.pk, self.pv, self.low = True, n, n, v, 0
            else:
                mask[i] = True
                if v > self.pv:
                    self.pv, self.pk = v, n
                if above[i]:
                    self.low = 0
                elif self.hyst == 0 or self.low >= lim:
                    evs.append(self._event(n))
                    vals.append(self.pv)
                    self.open, self.pv, self.low = False, 0.0, 0
                else:
                    self.low += 1
        self.n = n0 + Tc
        open_start = self.gs if self.open else -1
        if final:
            if self.open:
                evs.append(self._event(self.n))
                vals.append(self.pv)
                mask[max(0, self.gs - n0):] = True            # gate_mask[gate_start:n], this call's part
            self.reset()
        return dict(corr_mag=c, local_sum=local, corr_scaled=c * self.scale, thresh_scaled=local * self.tv,
                    above_threshold=above, metric_valid=valid, gate_mask=mask,
                    events=np.array(evs, np.int64).reshape(-1, 4), peak_values=np.array(vals, np.float64),
                    n_events=len(evs), open_gate_start=open_start, n0=n0)


ARRAYS = ("local_sum", "corr_scaled", "thresh_scaled", "above_threshold", "metric_valid")


def run_split(c, params, hysteresis, reference_length, split, flush=False):
    """The calls of one stream cut into pieces of `split` (sum = len(c)); the last piece is final, or with
    `flush` a Tc = 0 final call follows it.  Returns the list of per-call dicts."""
    assert sum(split) == len(c) and all(t >= 1 for t in split)
    m = ZCChunkModel(params, hysteresis, reference_length)
    out, at = [], 0
    for k, t in enumerate(split):
        out.append(m.push(c[at:at + t], final=(k == len(split) - 1 and not flush)))
        at += t
    if flush:
        out.append(m.push(c[:0], final=True))
    return out


def concat(calls):
    """Concatenated arrays, events and peak values of a list of per-call dicts."""
    r = {k: np.concatenate([d[k] for d in calls]) for k in ARRAYS + ("gate_mask",)}
    r["events"] = np.concatenate([d["events"] for d in calls]).reshape(-1, 4)
    r["peak_values"] = np.concatenate([d["peak_values"] for d in calls])
    return r


def mask_exception(calls):
    """The one sample where the concatenated gate_mask may be 0 and the one-shot mask 1: the start of a gate
    that the final call closed, when it lies before that call's first sample; else None."""
    last = calls[-1]
    g = last["open_gate_start"]
    return int(g) if g >= 0 and g < last["n0"] else None


def splits(n, W, seed):
    """The split list of the GPU tests for a stream of n samples (each a list of piece lengths)."""
    def pieces(t):
        s = [t] * (n // t)
        return s + ([n - sum(s)] if n - sum(s) else [])
    out = [[n], pieces(128), pieces(64), pieces(127), pieces(129), pieces(333), pieces(32)]
    if n >= 3:
        out.append([1, n - 2, 1])
    if W + 1 < n and W >= 2:
        out.append([W - 1, 1, 1, n - W - 1])                     # edges at W - 1, W and W + 1
    rng = np.random.default_rng(seed)
    k = int(rng.integers(2, 9))
    cuts = np.sort(rng.choice(np.arange(1, n), size=min(k, n - 1), replace=False))
    out.append(np.diff(np.concatenate(([0], cuts, [n]))).astype(int).tolist())
    return out
