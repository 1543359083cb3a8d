"""Host side of the native runner's learned-φ SF test phase (no GPU): the exported symbol, how
NativeEnvLoop.phi_test_phase slices and validates its arguments, and NativeEnvLoop.train's dispatch to it under
schedule "phi" at test_phase_steps' positions."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

A, D = 5, 6


def test_the_library_exports_the_phase():
    from sfx import _lib  # loads libsfx.so and resolves every symbol of SIGNATURES; no device needed

    assert "sfx_runner_phi_test_phase" in _lib.SIGNATURES
    fn = _lib.lib.sfx_runner_phi_test_phase
    assert fn.restype is C.c_int and len(fn.argtypes) == 12
    assert fn.argtypes[3] is C.c_float  # test_epsilon; no lr / wd: the reward mapper builds its own Adam
    # a null runner is refused by name before anything is touched
    assert fn(None, 1, 1, 0.0, None, 0, None, None, None, None, None, None) == -1
    assert "sfx_runner_phi_test_phase" in _lib.lib.sfx_last_error().decode()


class _FakeLib:
    """Stands in for libsfx: records the call and fills the outputs as a phase of full length would."""

    def __init__(self):
        self.calls = []

    def sfx_runner_phi_test_phase(self, r, E, horizon, eps, W, stride, Wb, ex, ret, loss, steps, acts):
        rec = dict(r=r, E=E, horizon=horizon, eps=eps, W=W, stride=stride, Wb=Wb, explore=None, acts=acts is not None)
        if ex is not None:
            rec["explore"] = np.ctypeslib.as_array(C.cast(ex, C.POINTER(C.c_int32)), shape=(E, horizon)).copy()
        np.ctypeslib.as_array(C.cast(steps, C.POINTER(C.c_int64)), shape=(max(E, 1),))[:E] = horizon
        np.ctypeslib.as_array(C.cast(ret, C.POINTER(C.c_double)), shape=(max(E, 1),))[:E] = np.arange(E) + 0.5
        if acts is not None:
            np.ctypeslib.as_array(C.cast(acts, C.POINTER(C.c_int64)), shape=(max(E, 1), max(horizon, 1)))[:E] = 3
        self.calls.append(rec)
        return 0


def _stub(episode_len=7):
    from sfx.runner import NativeEnvLoop

    lib = _FakeLib()

    def check(rc, what):
        assert rc == 0, what

    stub = types.SimpleNamespace(_C=C, _lib=lib, _check=check, _r="runner", episode_len=episode_len,
                                 eng=types.SimpleNamespace(device="cpu", A=A, d=D))
    return stub, lib, NativeEnvLoop.phi_test_phase


def test_phi_test_phase_slices_and_validates_like_test_phase():
    stub, lib, phase = _stub()
    E, stride = 3, D + 2
    W, Wb = torch.zeros(E, stride), torch.zeros(E)
    # explore: any integer array is converted to contiguous int32 of shape (E, horizon)
    ex64 = np.full((E, 4), -1, np.int64)
    ex64[1, 2] = A - 1
    ret, loss, steps, acts = phase(stub, W, Wb, horizon=4, test_epsilon=0.25, explore=ex64[:, ::1], want_actions=True)
    call = lib.calls[-1]
    assert (call["E"], call["horizon"], call["stride"], call["eps"]) == (E, 4, stride, 0.25)
    assert call["W"] == W.data_ptr() and call["Wb"] == Wb.data_ptr() and call["r"] == "runner"
    assert call["explore"].dtype == np.int32 and call["explore"].tolist() == ex64.tolist()
    assert ret.shape == (E,) and ret.dtype == np.float64 and loss.shape == (E,) and loss.dtype == np.float64
    assert steps.tolist() == [4] * E and steps.dtype == np.int64
    assert acts.shape == (E, 4) and acts.dtype == np.int64 and (acts == 3).all()
    # a Fortran-ordered view is made contiguous, row-major
    exf = np.asfortranarray(ex64.astype(np.int16))
    phase(stub, W, Wb, horizon=4, explore=exf)
    assert lib.calls[-1]["explore"].tolist() == ex64.tolist() and not lib.calls[-1]["acts"]
    # horizon defaults to the loop's episode_len; no explore: a null pointer, three outputs
    out = phase(stub, W, Wb)
    assert len(out) == 3 and lib.calls[-1]["horizon"] == 7 and lib.calls[-1]["explore"] is None
    n = len(lib.calls)
    for bad in (np.full((E, 5), -1), np.full((E + 1, 4), -1), np.full((E * 4,), -1)):
        with pytest.raises(ValueError, match=rf"explore: an int array \[{E}, 4\]"):
            phase(stub, W, Wb, horizon=4, explore=bad)
    over = ex64.copy()
    over[2, 0] = A
    with pytest.raises(ValueError, match=f"action >= A = {A}"):
        phase(stub, W, Wb, horizon=4, explore=over)
    # W: contiguous float32 [E, .] on the engine's device; Wb: E float32 elements there
    for badW in (torch.zeros(E, stride, dtype=torch.float64), torch.zeros(E * stride), torch.zeros(stride, E).t(),
                 np.zeros((E, stride), np.float32)):
        with pytest.raises(ValueError, match="W: a contiguous float32 tensor"):
            phase(stub, badW, Wb, horizon=4)
    for badWb in (torch.zeros(E + 1), torch.zeros(E, dtype=torch.float64), torch.zeros(2 * E)[::2], [0.0] * E):
        with pytest.raises(ValueError, match=f"Wb: a contiguous float32 tensor of E = {E} elements"):
            phase(stub, W, badWb, horizon=4)
    assert len(lib.calls) == n  # nothing reached the library


def test_train_evaluates_with_the_phi_phase_at_test_phase_steps():
    from sfx.runner import NativeEnvLoop, test_phase_steps

    class Stub:
        def __init__(self, schedule):
            self.schedule, self.log, self.t = schedule, [], 0

        def set_task(self, index):
            self.log.append(("task", index))
            self.t = 0

        def run(self, n):
            self.t += n

        def test_phase(self, W, **kw):
            self.log.append(("sf", self.t, W, kw))
            return (np.array([1.0, 3.0]),)

        def tsf_test_phase(self, W, **kw):
            self.log.append(("tsf", self.t, W, kw))
            return (np.array([2.0, 4.0]), None, None)

        def phi_test_phase(self, W, **kw):
            self.log.append(("phi", self.t, W, kw))
            return (np.array([5.0, 8.0]), None, None)

    kw = dict(Wb="Wb", horizon=6, test_epsilon=0.1)
    for n, ev in ((25, 10), (7, 1), (10, 10)):
        stub = Stub("phi")
        data = NativeEnvLoop.train(stub, [0, 2], n, "W", n_test_ev=ev, **kw)
        want = [t + 1 for t in test_phase_steps(n, ev)]
        assert want == [t + 1 for t in range(n) if t % ev == 0]
        for task in (0, 2):
            i = stub.log.index(("task", task))
            assert stub.log[i + 1:i + 1 + len(want)] == [("phi", t, "W", kw) for t in want]
        assert len(stub.log) == 2 * (1 + len(want)) and stub.t == n
        assert [float(v) for v in data] == [6.5] * (2 * len(want)) and all(isinstance(v, np.float32) for v in data)
    # the other schedules keep their phases
    for sched, tag in (("all", "sf"), ("active", "sf"), ("tsf", "tsf")):
        stub = Stub(sched)
        NativeEnvLoop.train(stub, 1, 25, "W", n_test_ev=10, horizon=6)
        assert [x[:2] for x in stub.log] == [("task", 0)] + [(tag, t) for t in (1, 11, 21)]
