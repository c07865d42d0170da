"""agx_iterate's failure protocol on the MI355X, single process.

With a recording exchange (tests/exchange_probe.py) the process is rank 0 of two and what it
posts is a log: a rank that fails posts, call by call, exactly what a healthy rank posts (its
peers are healthy ranks), a failing exchange ends the call, the first error's text wins.
Without an exchange: the context that failed is used again and gives, bit for bit, what a
fresh context gives.

Failures (tests/failure_decks.py), all through the library's own error word or a refused
phase -- the call returns, nothing faults:
  spin limit   AGX_SPIN_LIMIT=1: k_lusgs_kp (5-eq) and k_lusgs_pipe (7-eq), a bounded walk
  energy       thermally perfect explicit step at CFL 24: numpy says e < hf before the kernel
  refused      cfl = 0 without a time step: agx_phase_residual refuses, nothing is launched
The energy trigger does not reach the implicit solvers: their update is bounded by the
diagonal (x ~ R / (sum of spectral radii / 2) as dt grows), and on the CPU oracle the hot
two-block deck keeps min(e_new - hf) = 14.3 (LU-SGS), 14.3 (DPLUR), 14.3 (BLU-SGS) of
e = 14.6 at CFL 1e8, and 14.1 / 14.1 / 13.0 with a 60 % perturbation.  Their recovery is
held by the spin-limit and the refused-phase cases."""
import numpy as np
import pytest

from exchange_probe import RecordingExchange, allgathers, run_calls, swaps
from failure_decks import (ENERGY_MATCH, SPIN_MATCH, TP_CFL, TP_CFL_TRIGGER, WALK, deck,
                           energy_margin, local_states)
from parity_utils import rel_err, switches
from aither_amd.solver import Solver

pytestmark = pytest.mark.gpu

REFUSED_MATCH = "Neither dt or cfl"
TAIL = 2       # calls after the first failure


def _plan(trigger, case):
    """(deck name's CFL per call of the failing run, of the healthy run, environment of the
    failing context, the failure's text)"""
    d = case.deck
    if trigger == "spin":
        cfls = [d.cfl(nn) for nn in range(WALK + TAIL)]
        return cfls, cfls, {"AGX_SPIN_LIMIT": "1"}, SPIN_MATCH
    if trigger == "energy":
        return ([TP_CFL, TP_CFL_TRIGGER] + [TP_CFL] * TAIL, [TP_CFL] * (2 + TAIL), {},
                ENERGY_MATCH)
    cfl = d.cfl(0)
    return [cfl, 0.0] + [cfl] * TAIL, [cfl] * (2 + TAIL), {}, REFUSED_MATCH


def _logged_run(lib, case, env, cfls, initial, **kw):
    ex = RecordingExchange()
    with switches(env):
        sol = ex.attach(Solver(lib, case, rank=0, exchange=ex))
    try:
        failed, made = run_calls(sol, cfls, initial, **kw)
    finally:
        sol.close()
    return ex.marks(), failed, made


# ---- B: the failing rank posts what a healthy rank posts ---------------------------------
@pytest.mark.parametrize("eager", ["1", "0"])
@pytest.mark.parametrize("name,trigger,reupload", [
    ("kp", "spin", True), ("pipe", "spin", True), ("tp", "energy", True),
    ("kp", "refused", True), ("kp", "refused", False)])
def test_failing_rank_posts_what_a_healthy_rank_posts(oracle, name, trigger, reupload, eager):
    """The log of every call of a run with a failure -- the failing call and the calls after
    it on the same context -- is the log of the same call of the healthy run, slab for slab,
    and the failing call reaches its one all-gather.  After a failed call the initial state is
    uploaded again (the healthy run uploads after the same calls); reupload False: the caller
    goes on without touching the state, which a refused phase has left whole."""
    lib, case = deck(name, [0, 1])
    bad_cfls, good_cfls, env, match = _plan(trigger, case)
    if trigger == "energy":      # the trigger is numpy's verdict, the healthy CFL as well
        low = energy_margin(oracle, case, TP_CFL_TRIGGER, warm=[TP_CFL],
                            exchange=RecordingExchange())
        ok = energy_margin(oracle, case, TP_CFL, warm=[TP_CFL], exchange=RecordingExchange())
        print("min(e_new - hf): trigger", low, "healthy", ok)
        assert min(low.values()) < 0.0 < min(ok.values())
    initial = local_states(case) if reupload else {}
    eg = {"AGX_EAGER_GHOSTS": eager}
    bad, failed, made = _logged_run(lib, case, dict(env, **eg), bad_cfls, initial, tail=TAIL)
    assert failed, f"no call in {WALK} failed"
    assert all(match in msg for _, msg in failed), failed
    if trigger != "spin":
        assert [nn for nn, _ in failed] == [1]
    good, none, _ = _logged_run(lib, case, eg, good_cfls[:made], initial,
                                reupload_after={nn for nn, _ in failed})
    assert not none and len(good) == len(bad) == made
    for nn, (b, g) in enumerate(zip(bad, good)):
        print(nn, "failed" if nn in dict(failed) else "ok", [e[1] for e in swaps(b)],
              "healthy", [e[1] for e in swaps(g)])
    for nn, (b, g) in enumerate(zip(bad, good)):
        assert b == g, (nn, "failing run", b, "healthy run", g)
        assert len(allgathers(b)) == 1 and b[-1][0] == "allgather", (nn, b)


# ---- the AGX_XCHG rules ------------------------------------------------------------------
def _first_call(lib, case, eager, cfl=None, **knobs):
    ex = RecordingExchange()
    with switches(AGX_EAGER_GHOSTS=eager):
        sol = ex.attach(Solver(lib, case, rank=0, exchange=ex))
    ex.arm(**knobs)
    sol.store_time_n(0)
    try:
        sol.iterate(0, case.deck.cfl(0) if cfl is None else cfl)
        msg = None
    except RuntimeError as err:
        msg = str(err)
    last = lib.last_error().decode()
    sol.close()
    (call,) = ex.marks()
    return call, msg, last


@pytest.mark.parametrize("eager", ["1", "0"])
def test_exchange_failure_ends_the_call(eager):
    """A swap that fails -- the state exchange, one in the sweeps, the last of the call (with
    eager ghosts the fill queued for the next call) -- fails the call by name; nothing is
    posted after it, neither a swap nor the all-gather: the peers cannot be helped.  The
    text is the exchange's also when an earlier call left another one behind."""
    lib, case = deck("kp", [0, 1])
    healthy, msg, _ = _first_call(lib, case, eager)
    assert msg is None and len(allgathers(healthy)) == 1
    n = len(swaps(healthy))
    assert n == (5 if eager == "1" else 4)      # state, forward, backward, final (, next state)
    _, msg, _ = _first_call(lib, case, eager, cfl=0.0)      # leaves its text in agx_last_error
    assert REFUSED_MATCH in msg
    for k in (1, 2, n):
        call, msg, _ = _first_call(lib, case, eager, fail_swap_at=k)
        assert msg is not None and "the exchange's swap operation failed" in msg, (k, msg)
        assert call == healthy[:k], (k, call)
    call, msg, _ = _first_call(lib, case, eager, raise_in_swap_at=2)
    assert "swap operation failed" in msg and "swap 2 raised" in msg and call == healthy[:2]


@pytest.mark.parametrize("eager", ["1", "0"])
def test_first_error_wins_over_a_failing_exchange(eager):
    """A refused phase, then a failing exchange: the call ends there, and agx_last_error
    holds the refusal, not the exchange's text."""
    lib, case = deck("kp", [0, 1])
    call, msg, last = _first_call(lib, case, eager, cfl=0.0, fail_swap_at=2)
    assert REFUSED_MATCH in msg and REFUSED_MATCH in last and "swap" not in last
    assert len(swaps(call)) == 2 and not allgathers(call)


def test_failing_allgather_fails_the_call_by_name():
    lib, case = deck("kp", [0, 1])
    _, msg, _ = _first_call(lib, case, "1", cfl=0.0)        # (a stale text to overwrite)
    assert REFUSED_MATCH in msg
    call, msg, _ = _first_call(lib, case, "1", fail_allgather=True)
    assert "the exchange's allgather operation failed" in msg
    assert len(allgathers(call)) == 1 and call[-1][0] == "allgather"


# ---- D: recovery on the same context -----------------------------------------------------
def _iterate(sol, nn, cfl):
    sol.store_time_n(nn)
    l2, linf, mres = sol.iterate(0, cfl)
    return (l2.copy(), (linf.linf, linf.block, linf.i, linf.j, linf.k, linf.eqn), mres)


def _snapshot(sol, case):
    g = case.ng
    return {gb: (sol.download("state", gb)[g:-g, g:-g, g:-g], sol.download("residual", gb))
            for gb in sol.block_ids}


# The scalar LU-SGS path of the 5-equation library (the kp deck) knows a context's past, failure
# or none: every x in the diagonal-ordered arrays carries the tag of the launch that wrote it in
# its two low mantissa bits (<= 3 ulp, 7e-16 relative), and the tag follows the
# block's epoch, which every earlier call has advanced.  Measured on the kp deck, a context that
# has made ONE healthy call and had the initial state uploaded again against a fresh one:
#   first call   L2, L-inf (formed of the uploaded state alone) bit for bit; the matrix residual,
#                formed of x as stored, 2.64271175266545e-10 against 2.642711752665447e-10;
#   second call  L2 equal to the 9 digits printed, not to the last bit: the update adds the
#                tagged x to a state ~1e5 times larger, where 3 ulp of x decide a rounding of the
#                state in a few cells of 1e5 (one ulp, 2.2e-16), and the residual of that state
#                is a difference of fluxes 1e2..1e3 times larger than itself.  After it: state
#                1.6e-15, residual 1.2e-14, L2 8.9e-16, matrix residual 2.4e-15 (relative).
# So on that deck the first call's L2 and L-inf are held bit for bit and everything that has
# seen x -- the matrix residual, the state and the residual after it, later norms -- to
# TAG_RTOL: three orders above the tag and the ulp, for the cancellation in A x - b after one
# sweep and in the flux balance; the tolerance test_matrix_residual_forms_agree holds two
# orders of the same sum to.  A stale flag is a different buffer or a skipped pass: O(1).
# The explicit path and the 7-equation library carry no tags: bit for bit throughout.
TAG_RTOL = 1e-12


def _assert_same(got, want, norms_got, norms_want, tagged=False):
    """tagged: the kp deck, see TAG_RTOL.  A single call (the spin-limit recovery) keeps its
    state and residual bit for bit as well."""
    assert len(norms_got) == len(norms_want)
    loose = tagged and len(norms_want) > 1
    if tagged:      # the figures, before anything is asserted
        for n, ((l2g, _, mg), (l2w, _, mw)) in enumerate(zip(norms_got, norms_want)):
            print("call", n, "L2 rel", float(np.abs(l2g / l2w - 1.0).max()), "mres rel",
                  abs(mg / mw - 1.0))
        for gb in want:
            print("block", gb, "state rel", rel_err(got[gb][0], want[gb][0]), "residual rel",
                  rel_err(got[gb][1], want[gb][1]))
    for n, ((l2g, linfg, mg), (l2w, linfw, mw)) in enumerate(zip(norms_got, norms_want)):
        if tagged and n > 0:
            assert np.allclose(l2g, l2w, rtol=TAG_RTOL, atol=0.0), (n, l2g, l2w)
            assert abs(linfg[0] - linfw[0]) <= TAG_RTOL * linfw[0] and linfg[1:] == linfw[1:]
        else:
            assert np.array_equal(l2g, l2w) and linfg == linfw, (n, l2g, l2w, linfg, linfw)
        if tagged:
            assert mw > 0.0 and abs(mg - mw) <= TAG_RTOL * mw, (n, mg, mw)
        else:
            assert mg == mw, (n, mg, mw)
    for gb in want:
        for q, what in enumerate(("state", "residual")):
            if loose:
                assert rel_err(got[gb][q], want[gb][q]) <= TAG_RTOL, (what, gb)
            else:
                assert np.array_equal(got[gb][q], want[gb][q]), (what, gb)


def _upload(sol, initial):
    for gb, st in initial.items():
        sol.upload("state", gb, st)


@pytest.mark.parametrize("eager", ["1", "0"])
@pytest.mark.parametrize("name,trigger", [("tp", "energy"), ("kp", "refused"),
                                          ("pipe", "refused")])
def test_deterministic_failure_then_the_same_context_as_a_fresh_one(oracle, name, trigger, eager):
    """One healthy call, the failing call, the initial state uploaded again, two calls:
    state, residual, L2 and L-inf of those two are a fresh context's, bit for bit; the matrix
    residual as well, but on the kp deck, where x carries its launch's tag (TAG_RTOL)."""
    lib, case = deck(name)
    initial = local_states(case)
    good = TP_CFL if trigger == "energy" else case.deck.cfl(0)
    bad, match = (TP_CFL_TRIGGER, ENERGY_MATCH) if trigger == "energy" else (0.0, REFUSED_MATCH)
    if trigger == "energy":
        low = energy_margin(oracle, case, bad, warm=[good])
        print("min(e_new - hf):", low)
        assert min(low.values()) < 0.0
    with switches(AGX_EAGER_GHOSTS=eager):
        fresh, sol = Solver(lib, case), Solver(lib, case)
    want_norms = [_iterate(fresh, nn, good) for nn in range(2)]
    want = _snapshot(fresh, case)
    fresh.close()
    _iterate(sol, 0, good)
    with pytest.raises(RuntimeError, match=match):
        _iterate(sol, 1, bad)
    _upload(sol, initial)
    got_norms = [_iterate(sol, nn, good) for nn in range(2)]
    got = _snapshot(sol, case)
    sol.close()
    _assert_same(got, want, got_norms, want_norms, tagged=name == "kp")


@pytest.mark.parametrize("name", ["kp", "pipe"])
def test_spin_limit_then_the_same_context_recovers(name):
    """The context created with AGX_SPIN_LIMIT=1 is kept after its failure (k_lusgs_kp; and
    k_lusgs_pipe on two blocks, whose progress words are set up afresh): the initial state
    uploaded again, the first call that succeeds -- of WALK at most -- gives the state, the
    residual, L2 and L-inf of a fresh context's first iteration under the default limit, bit
    for bit (the matrix residual of the kp deck: see TAG_RTOL)."""
    lib, case = deck(name)
    initial = local_states(case)
    cfl = case.deck.cfl(0)
    fresh = Solver(lib, case)
    want_norms = [_iterate(fresh, 0, cfl)]
    want = _snapshot(fresh, case)
    fresh.close()
    with switches(AGX_SPIN_LIMIT="1"):
        sol = Solver(lib, case)
    try:
        with pytest.raises(RuntimeError, match=SPIN_MATCH):
            for nn in range(WALK):
                _iterate(sol, nn, case.deck.cfl(nn))
        got_norms = None
        for _ in range(WALK):
            _upload(sol, initial)
            try:
                got_norms = [_iterate(sol, 0, cfl)]
                break
            except RuntimeError as err:
                assert SPIN_MATCH in str(err)
        if got_norms is None:
            pytest.skip(f"no call of {WALK} got through under AGX_SPIN_LIMIT=1")
        got = _snapshot(sol, case)
    finally:
        sol.close()
    _assert_same(got, want, got_norms, want_norms, tagged=name == "kp")
