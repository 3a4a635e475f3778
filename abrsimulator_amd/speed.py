"""A closed-loop play-speed controller, evaluated on the device (include/abr_env.h: abr_speed_rule).

The reference asks ``speed_controller.get_next_speed()`` at the first playing tick of every played chunk
(Simulator.py:176-177) and ships no controller of its own (D8).  ``LatencySpeedController`` is the build's: a stateless,
piecewise-constant table over the instant latency and the buffer level at that tick, comparisons only.  At the first
playing tick of a played chunk

    lat = global_time - play_time      (the reference's instant_latency, :179)
    buf = buffer_level                 (after a download that completes on this tick, before this tick's drain)
    i   = number of q with lat >= latency_thresholds[q]
    j   = number of r with buf >= buffer_thresholds[r]

and the chunk plays at ``speeds[i][j]``.  The table runs inside the environment kernels: hand it to
``BatchedABREnv(..., speed=ctl)``, ``BatchedABREnv.set_speed_controller`` or ``Simulator(abr, speed_controller=ctl)``.
"""
import math

from . import _lib

MAX_THRESHOLDS = _lib.SPEED_RULE_MAX_THR


def _check_thresholds(name, thr):
    thr = tuple(float(x) for x in thr)
    if len(thr) > MAX_THRESHOLDS:
        raise ValueError(f"{name}: at most {MAX_THRESHOLDS} thresholds, got {len(thr)}")
    if not all(math.isfinite(x) for x in thr):
        raise ValueError(f"{name} must be finite")
    if any(not (b > a) for a, b in zip(thr, thr[1:])):
        raise ValueError(f"{name} must be strictly ascending")
    return thr


class LatencySpeedController:
    """speeds: (len(latency_thresholds) + 1) rows of (len(buffer_thresholds) + 1) play speeds, finite and > 0."""

    def __init__(self, latency_thresholds=(), buffer_thresholds=(), speeds=((1.0,),)):
        self.latency_thresholds = _check_thresholds("latency_thresholds", latency_thresholds)
        self.buffer_thresholds = _check_thresholds("buffer_thresholds", buffer_thresholds)
        rows = [tuple(float(v) for v in r) for r in speeds]
        nl, nb = len(self.latency_thresholds), len(self.buffer_thresholds)
        if len(rows) != nl + 1 or any(len(r) != nb + 1 for r in rows):
            raise ValueError(f"speeds must be {nl + 1} rows of {nb + 1} values "
                             "(one more than the latency / buffer thresholds)")
        if not all(math.isfinite(v) and v > 0.0 for r in rows for v in r):
            raise ValueError("speeds must be finite and > 0")
        self.speeds = tuple(rows)

    @classmethod
    def catch_up(cls, target_latency, fast=1.1, low_buffer=None, slow=0.9):
        """Play at `fast` while the latency is at or above `target_latency`, else at 1.0; with `low_buffer`, play at
        `slow` whenever the buffer is below it (slowing down near a rebuffer wins over catching up)."""
        if low_buffer is None:
            return cls((target_latency,), (), ((1.0,), (fast,)))
        return cls((target_latency,), (low_buffer,), ((slow, 1.0), (slow, fast)))

    def speed_for(self, latency, buffer_level):
        """The rule itself, in Python floats (what the device computes for these inputs)."""
        i = sum(1 for t in self.latency_thresholds if latency >= t)
        j = sum(1 for t in self.buffer_thresholds if buffer_level >= t)
        return self.speeds[i][j]

    def to_struct(self):
        """include/abr_env.h: abr_speed_rule."""
        r = _lib.SpeedRule()
        r.n_lat, r.n_buf = len(self.latency_thresholds), len(self.buffer_thresholds)
        for q, t in enumerate(self.latency_thresholds):
            r.lat_thr[q] = t
        for q, t in enumerate(self.buffer_thresholds):
            r.buf_thr[q] = t
        for i, row in enumerate(self.speeds):
            for j, v in enumerate(row):
                r.speed[i][j] = v
        return r

    def get_next_speed(self):
        raise RuntimeError("LatencySpeedController is evaluated on the device, at the first playing tick of every played "
                           "chunk, from that lane's latency and buffer level: pass it to BatchedABREnv(..., speed=ctl), "
                           "BatchedABREnv.set_speed_controller(ctl) or Simulator(abr, speed_controller=ctl)")

    def __repr__(self):
        return (f"LatencySpeedController(latency_thresholds={self.latency_thresholds}, "
                f"buffer_thresholds={self.buffer_thresholds}, speeds={self.speeds})")
