"""The recording exchange of tests/exchange_probe.py on the CPU oracle: one process as rank 0
of two.  What a healthy iterate() posts, per call, is what agx_iterate documents -- the state
exchange, per sweep the update exchanges, the final one, one all-gather -- and the same on
two runs; a swap that fails or raises fails the call with a message."""
import pytest

from aither_amd import abi
from aither_amd.case import synthetic
from aither_amd.solver import Solver
from exchange_probe import RecordingExchange, allgathers, swaps
from test_distributed_cpu import KW

DIMS = (6, 5, 4)


def _case(kind):
    return synthetic.stacked_blocks_case(DIMS, nblocks=2, axis="k", stretch=1.1,
                                         ranks=[0, 1], **KW[kind])


def _run(oracle, kind, steps=2, **knobs):
    ex = RecordingExchange(**knobs)
    sol = ex.attach(Solver(oracle, _case(kind), rank=0, exchange=ex))
    try:
        for nn in range(steps):
            sol.step(nn)
    finally:
        counts = {what: oracle.halo_count(sol.ctx, sol.conn_ids[0], what)
                  for what in (abi.HALO_STATE, abi.HALO_UPDATE)}
        sol.close()
    return ex, counts, sol.case.deck


def _documented(deck, counts):
    """The exchanges of one ora_iterate / agx_iterate call of an Euler deck (no velocity
    gradients, no turbulence variables): slab counts in order."""
    want = [counts[abi.HALO_STATE]]
    if deck.is_implicit():
        per_sweep = 2 if deck.matrix_solver in ("lusgs", "blusgs") else 1
        want += [counts[abi.HALO_UPDATE]] * (per_sweep * deck.matrix_sweeps + 1)
    return want


@pytest.mark.parametrize("kind", ["rk4", "lusgs", "dplur"])
def test_healthy_log_is_documented_and_repeatable(oracle, kind):
    ex, counts, deck = _run(oracle, kind)
    calls = ex.marks()
    # (rk4: the four stages are the deck's nonlinear iterations)
    assert len(calls) == 2 * deck.nonlinear_iterations == (8 if kind == "rk4" else 2)
    assert counts[abi.HALO_STATE] > 0 and counts[abi.HALO_UPDATE] > 0
    want = _documented(deck, counts)
    for call in calls:
        # one slab per swap: peer 1, tag 0 (the one connection to the other rank)
        assert [e[1] for e in swaps(call)] == [((1, 0, n),) for n in want], call
        assert len(allgathers(call)) == 1 and call[-1][0] == "allgather", call
    again, _, _ = _run(oracle, kind)
    assert again.marks() == calls


@pytest.mark.parametrize("kind,at", [("rk4", 1), ("lusgs", 1), ("lusgs", 3), ("dplur", 6)])
@pytest.mark.parametrize("knob", ["fail_swap_at", "raise_in_swap_at"])
def test_failing_swap_fails_the_call_with_a_message(oracle, kind, at, knob):
    with pytest.raises(RuntimeError, match="swap operation failed") as info:
        _run(oracle, kind, **{knob: at})
    if knob == "raise_in_swap_at":      # the transport's own exception is not swallowed
        assert isinstance(info.value.__cause__, TimeoutError)
        assert f"swap {at} raised" in str(info.value)
    else:
        assert info.value.__cause__ is None


def test_failing_allgather_fails_the_call_with_a_message(oracle):
    with pytest.raises(RuntimeError, match="allgather operation failed"):
        _run(oracle, "lusgs", fail_allgather=True)


def test_failed_call_logs_nothing_after_the_failing_swap(oracle):
    """The oracle has no failure protocol: the call ends at the failing swap."""
    ex = RecordingExchange(fail_swap_at=3)
    sol = ex.attach(Solver(oracle, _case("lusgs"), rank=0, exchange=ex))
    with pytest.raises(RuntimeError, match="swap operation failed"):
        sol.step(0)
    sol.close()
    (call,) = ex.marks()
    assert len(swaps(call)) == 3 and not allgathers(call)


def test_dist_exchange_callbacks_return_failure_when_they_raise():
    """DistExchange without a process group: torch.distributed raises inside the callback;
    the callback returns 1 and keeps the exception instead of printing it and returning 0."""
    import ctypes as C
    import numpy as np
    from aither_amd.solver import DistExchange
    ex = DistExchange(2)
    buf = np.zeros(8)
    slab = (abi.Slab * 1)()
    slab[0].peer, slab[0].tag, slab[0].count = 1, 0, 8
    slab[0].send = slab[0].recv = buf.ctypes.data_as(abi.c_dp)
    assert ex.struct.swap(None, 1, slab, None) == 1
    assert ex.pending is not None
    ex.pending = None
    out = np.zeros(32)
    assert ex.struct.allgather(None, buf.ctypes.data, out.ctypes.data, 64, None) == 1
    assert ex.pending is not None
