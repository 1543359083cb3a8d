"""What tools/test_phase.py and tools/tsf_test_phase.py share: the agents' logger, the timing of a test phase and
the two tools' command line.  Kept apart from both so that either tool works on its own."""
from __future__ import annotations

import time

import torch


class Log:
    """The agent's logger, keeping its lines; ``tagged`` for the TSF agents, which log two kinds of line."""

    def __init__(self, tagged=False):
        self.lines, self.tagged = [], tagged

    def log_target_error_progress(self, d):
        self.lines.append(("err", d) if self.tagged else d)

    def log_omegas_learning_rate(self, lr, i, t):
        self.lines.append(("lr", lr, i, t))


def timed(run, close, n, phases, path) -> dict:
    """One warm-up phase (graphs captured), ``phases`` phases of ``n`` env steps in all under the clock, then
    ``close()``: an entry of bench.py's ``other_workloads``."""
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(phases):
        run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    close()
    return {"value": round(n / dt, 2), "unit": "test env steps/s", "ms_per_step": round(1000.0 * dt / n, 4),
            "steps": n, "dtype": "fp32", "path": path}


def main(measure):
    """``python tools/test_phase.py`` or ``python tools/tsf_test_phase.py``: the phase both ways, one JSON line each."""
    import json

    for ls in (False, True):
        print(json.dumps({"lockstep" if ls else "sequential": measure(ls)}), flush=True)
