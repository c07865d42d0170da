"""A recording agx_exchange (include/aither_gfx950.h) for ONE process that plays rank 0 of
two: it never blocks, so a rank that posts an exchange too many -- or one too few -- shows as
a wrong log instead of a hang.

swap mirrors every slab (recv = send: the ghost cells across the connection take the rank's
own boundary cells, finite and physical), allgather copies this rank's record into every
rank's slot (the layout of the record is the library's own business).  Both are logged:
("swap", ((peer, tag, count), ...)) and ("allgather", nbytes).  The knobs make the n-th swap
since arm() return 1 or raise, or every allgather return 1; a callback that raises returns 1
and keeps the exception in `pending`, as aither_amd.solver.DistExchange does.

Works with the product library and with the CPU oracle (host buffers either way)."""
import ctypes as C

from aither_amd import abi


class RecordingExchange:
    def __init__(self, nranks=2, fail_swap_at=None, fail_allgather=False,
                 raise_in_swap_at=None):
        self.nranks = nranks
        self.log = []          # ("mark",) | ("swap", slabs) | ("allgather", nbytes)
        self.pending = None    # the exception a callback raised (read by Solver)
        self.arm(fail_swap_at, fail_allgather, raise_in_swap_at)
        self._swap = abi.SWAP_FN(self.swap)
        self._allgather = abi.ALLGATHER_FN(self.allgather)
        self.struct = abi.Exchange(None, self._swap, self._allgather, nranks, 1)

    def arm(self, fail_swap_at=None, fail_allgather=False, raise_in_swap_at=None):
        """Set the knobs; the swaps are counted from 1 from here on."""
        self.fail_swap_at, self.raise_in_swap_at = fail_swap_at, raise_in_swap_at
        self.fail_allgather = fail_allgather
        self.nswap = 0

    # -- the two callbacks ----------------------------------------------------------------
    def swap(self, user, n, slabs, stream):
        try:
            self.nswap += 1
            self.log.append(("swap", tuple((int(slabs[q].peer), int(slabs[q].tag),
                                            int(slabs[q].count)) for q in range(n))))
            if self.nswap == self.raise_in_swap_at:
                raise TimeoutError(f"recording exchange: swap {self.nswap} raised")
            if self.nswap == self.fail_swap_at:
                return 1
            for q in range(n):
                sl = slabs[q]
                if sl.count > 0:
                    C.memmove(sl.recv, sl.send, 8 * int(sl.count))
            return 0
        except Exception as exc:      # (a ctypes callback that raises would return 0)
            self.pending = exc
            return 1

    def allgather(self, user, send, recv, nbytes, stream):
        try:
            self.log.append(("allgather", int(nbytes)))
            if self.fail_allgather:
                return 1
            for r in range(self.nranks):
                C.memmove(recv + r * int(nbytes), send, int(nbytes))
            return 0
        except Exception as exc:
            self.pending = exc
            return 1

    # -- the log per agx_iterate call --------------------------------------------------------
    def mark(self):
        self.log.append(("mark",))

    def attach(self, sol):
        """Every sol.iterate() from here on opens a new entry of marks()."""
        inner = sol.iterate

        def iterate(mm, cfl):
            self.mark()
            return inner(mm, cfl)
        sol.iterate = iterate
        return sol

    def marks(self):
        """The log split at the marks: one list of entries per agx_iterate call (what came
        before the first mark -- set-up -- is left out)."""
        calls = []
        for entry in self.log:
            if entry[0] == "mark":
                calls.append([])
            elif calls:
                calls[-1].append(entry)
        return calls


def swaps(call):
    return [e for e in call if e[0] == "swap"]


def allgathers(call):
    return [e for e in call if e[0] == "allgather"]


def run_calls(sol, cfls, initial, reupload_after=(), tail=None):
    """One agx_iterate call (store_time_n, iterate(0, cfl)) per entry of cfls on a Solver
    with the exchange attached.  A call that fails is caught and `initial` ({global block:
    state}) uploaded again; so it is after the calls listed in reupload_after, with which a
    healthy run mirrors a failing one.  tail: stop that many calls after the first failure
    (a bounded walk towards a failure that does not strike at a fixed call).
    Returns [(call index, message)] of the failed calls and the number of calls made."""
    failed, made = [], 0
    for nn, cfl in enumerate(cfls):
        if tail is not None and failed and nn > failed[0][0] + tail:
            break
        sol.store_time_n(nn)
        made += 1
        try:
            sol.iterate(0, cfl)
        except RuntimeError as err:
            failed.append((nn, str(err)))
        if (failed and failed[-1][0] == nn) or nn in reupload_after:
            for gb, st in initial.items():
                sol.upload("state", gb, st)
    return failed, made
