"""Host-side mirror of the reference's time-step loop around the C-ABI.

`Solver` plays the role of main.cpp:231-302 + logFileManager: it owns one
library context, uploads a Case (aither_amd.case.builder.Case), and calls
store_time_n / iterate exactly where the reference calls
mgSolution::StoreOldSolution (main.cpp:239) and mgSolution::Iterate
(main.cpp:249).  Residual normalisation follows PrintResiduals
(src/output.cpp:1028-1087).  PyTorch is not involved here; the same class
drives the product library ("agx_") and, in tests only, the CPU oracle
("ora_").
"""
import ctypes as C
import math
import numpy as np

from . import abi
from .case import builder as _b
from .case import geometry as _geo

EPS = 1.0e-30  # macros.hpp.in:20


def pool_bins(parts):
    """Join collapsed statistics (Solver.stats_collapse) of blocks that share the remaining
    directions, or of ranks: parts is a list of (volume, means, covs) with volume an array over
    the bins, means {name: array} and covs {key: array} of that shape; a key is a pair
    (a, b) of names in means or a second moment of abi.STAT_PAIRS ("cov_uv", ...).  Joined in
    list order by the pairwise form, r = V2 / (V1 + V2), delta = M2 - M1:
        M = M1 + r delta;  cov = cov1 + r (cov2 - cov1) + (V1 r / V) delta_a delta_b
    in numpy float64.  Parts with bit-identical means and covs return them bit for bit.
    Returns (volume, means, covs)."""
    vol, means, covs = parts[0]
    vol = np.array(vol, dtype=np.float64)
    means = {n: np.array(m, dtype=np.float64) for n, m in means.items()}
    covs = {k: np.array(c, dtype=np.float64) for k, c in covs.items()}
    for vol2, means2, covs2 in parts[1:]:
        vol2 = np.asarray(vol2, dtype=np.float64)
        total = vol + vol2
        some = total != 0.0
        r = np.where(some, vol2 / np.where(some, total, 1.0), 0.0)
        cf = np.where(some, vol * r / np.where(some, total, 1.0), 0.0)
        d = {n: np.asarray(means2[n], dtype=np.float64) - means[n] for n in means}
        for k in covs:
            a, b = k if isinstance(k, tuple) else abi.STAT_PAIRS[k]
            covs[k] = covs[k] + r * (np.asarray(covs2[k], dtype=np.float64) - covs[k]) \
                + cf * (d[a] * d[b])
        for n in means:
            means[n] = means[n] + r * d[n]
        vol = total
    return vol, means, covs


def pool_fluxes(parts, tags=None, bc_types=None):
    """Add the boundary fluxes of blocks, or of ranks: parts is a list of
    (Solver.flux_surfaces(gb), Solver.surface_fluxes(gb)), one per block, of any ranks.
    Returns {name: float}, every surface that passes the filters added in list order (block,
    then surface) in float64.  tags / bc_types: only surfaces whose BC tag / BC type is listed.
    Without filters the two sides of every connection both of whose blocks are in `parts`
    cancel (the inviscid values to rounding, the viscous ones up to the faces on the rim of
    the patch, which each block evaluates with its own edge ghost cells), and what is left is
    the flux through the outer boundary.  Right after a residual the pooled net flux of an
    equation is the sum of the blocks' residual sums (Solver.block_budget) in any case."""
    total = {}
    for surfs, vals in parts:
        for q, s in enumerate(surfs):
            if tags is not None and s["tag"] not in tags:
                continue
            if bc_types is not None and s["bc_type"] not in bc_types:
                continue
            for n, v in vals.items():
                total[n] = total.get(n, 0.0) + float(v[q])
    return total


def pool_series(parts, records=None):
    """Join located points (Solver.series_locate) of blocks, or of ranks: parts is a list of
    [P, 5] arrays (gb, i, j, k, d2) for the same P points.  Per point the entry with the
    smallest d2 is kept, the lowest gb among equal ones, in the caller's order of points.
    Returns [P, 5].
    records: the sampled rows to go with it -- a list (one entry per rank) of
    {gb: (t, values)} of Solver.series_rows for blocks planned by
    Solver.series_plan_located(where, ...) with the joined `where`; then the return is
    (where, t[rows], values[rows, V, P]) with the points back in the caller's order.  Every
    record must hold the same rows (the ranks sample in step)."""
    where = np.array(parts[0], dtype=np.float64)
    for part in parts[1:]:
        part = np.asarray(part, dtype=np.float64)
        take = (part[:, 4] < where[:, 4]) | ((part[:, 4] == where[:, 4]) &
                                             (part[:, 0] < where[:, 0]))
        where[take] = part[take]
    if records is None:
        return where
    t = values = None
    for rank_records in records:
        for gb, (tb, vb) in rank_records.items():
            at = np.flatnonzero(where[:, 0] == gb)
            if values is None:
                t = np.array(tb, dtype=np.float64)
                values = np.full((vb.shape[0], vb.shape[1], len(where)), np.nan)
            assert np.array_equal(t, tb), "the records of the blocks hold different rows"
            values[:, :, at] = vb
    return where, t, values


def pool_spectra(parts):
    """Join the spectra (Solver.spectra) of blocks, or of ranks, that share N and the bins:
    parts is a list of (values, W, lines) -- values[nspec, ..., nmode], the sum of weights and
    the lines of a bin (the product of the block's pooled extents).  A part weighs lines x W;
    joined in list order by the pairwise form of pool_bins, r = g2 / (g1 + g2):
        S = S1 + r (S2 - S1)
    in numpy float64, so parts with bit-identical values return them bit for bit.  Lines are
    never lengthened: a spectrum stays that of a block's own N.  Returns (values, weight)."""
    values, W, lines = parts[0]
    values = np.array(values, dtype=np.float64)
    weight = float(lines) * float(W)
    for v2, W2, lines2 in parts[1:]:
        g2 = float(lines2) * float(W2)
        total = weight + g2
        r = g2 / total if total != 0.0 else 0.0
        values = values + r * (np.asarray(v2, dtype=np.float64) - values)
        weight = total
    return values, weight


def correlation(spectrum, n):
    """The circular two-point correlation of a one-sided spectrum (Solver.spectra, last axis
    the modes 0 ... n // 2 of lines of n cells): R(r) = sum_m S_m cos(2 pi m r / n) for
    r = 0 ... n - 1, last axis r.  R(0) is the mean of x_a x_b (Parseval); entry m = 0 carries
    the product of the means, so R is the correlation of the values, not of the fluctuations
    (drop S_0 for those).  Host numpy; the twiddle index m r mod n is formed in integers."""
    s = np.asarray(spectrum, dtype=np.float64)
    m = np.arange(s.shape[-1])
    q = np.outer(m, np.arange(n)) % n
    return s @ np.cos(2.0 * np.pi * q / n)


class DistExchange:
    """An agx_exchange (include/aither_gfx950.h) on torch.distributed
    point-to-point with HOST buffers: what an MPI adapter would pass
    (MPI_Sendrecv / MPI_Allgather), here over gloo for the multi-process tests.
    The production transport is the library's own RCCL one
    (agx_rccl_exchange_create).

    A ctypes callback that raises would print the exception and return 0 -- a transport that
    timed out would look like a completed exchange.  So both callbacks return 1 on an
    exception and keep it in `pending`; Solver raises it with the failed call."""

    def __init__(self, world, group=None):
        import torch
        import torch.distributed as dist
        self.torch, self.dist, self.world, self.group = torch, dist, world, group
        self.pending = None
        self._swap = abi.SWAP_FN(self._guard(self.swap))
        self._allgather = abi.ALLGATHER_FN(self._guard(self.allgather))
        self.struct = abi.Exchange(None, self._swap, self._allgather, world, 1)

    def _guard(self, fn):
        def guarded(*args):
            try:
                return fn(*args)
            except Exception as exc:
                self.pending = exc
                return 1
        return guarded

    def _view(self, ptr, n, dtype):
        ct = C.c_double if dtype == np.float64 else C.c_uint8
        arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(max(int(n), 1),))
        return self.torch.from_numpy(arr)[:int(n)]

    def swap(self, user, n, slabs, stream):
        reqs = []
        for q in range(n):
            sl = slabs[q]
            if sl.count <= 0:
                continue
            reqs.append(self.dist.isend(self._view(sl.send, sl.count, np.float64),
                                        sl.peer, tag=sl.tag, group=self.group))
            reqs.append(self.dist.irecv(self._view(sl.recv, sl.count, np.float64),
                                        sl.peer, tag=sl.tag, group=self.group))
        for r in reqs:
            r.wait()
        return 0

    def allgather(self, user, send, recv, nbytes, stream):
        mine = self._view(send, nbytes, np.uint8).clone()
        parts = [self.torch.empty(nbytes, dtype=self.torch.uint8) for _ in range(self.world)]
        self.dist.all_gather(parts, mine, group=self.group)
        out = self._view(recv, nbytes * self.world, np.uint8)
        for r, p in enumerate(parts):
            out[r * nbytes:(r + 1) * nbytes] = p
        return 0


class DeviceSetup:
    """The volume-sized parts of the grid set-up in the library:
    plot3dBlock's metrics (agx_plot3d_metrics) and the nearest-wall search of
    CalcWallDistance (agx_nearest_wall_distance).  Handed to case.builder.build_case."""

    def __init__(self, api, device=0):
        self.api = api
        self.ctx = C.c_void_p()
        api.check(api.ctx_create(device, 0, C.byref(self.ctx)), "ctx_create")

    def close(self):
        if self.ctx:
            self.api.ctx_destroy(self.ctx)
            self.ctx = None

    def metrics(self, coords):
        x = np.ascontiguousarray(coords, dtype=np.float64)
        nk, nj, ni = (s - 1 for s in x.shape[:3])
        out = dict(vol=np.empty((nk, nj, ni, 1)), center=np.empty((nk, nj, ni, 3)),
                   farea_i=np.empty((nk, nj, ni + 1, 4)), farea_j=np.empty((nk, nj + 1, ni, 4)),
                   farea_k=np.empty((nk + 1, nj, ni, 4)), fcen_i=np.empty((nk, nj, ni + 1, 3)),
                   fcen_j=np.empty((nk, nj + 1, ni, 3)), fcen_k=np.empty((nk + 1, nj, ni, 3)))
        p = lambda a: a.ctypes.data_as(abi.c_dp)
        self.api.check(self.api.plot3d_metrics(
            self.ctx, ni, nj, nk, p(x), p(out["vol"]), p(out["center"]), p(out["farea_i"]),
            p(out["farea_j"]), p(out["farea_k"]), p(out["fcen_i"]), p(out["fcen_j"]),
            p(out["fcen_k"])), "plot3d_metrics")
        return out

    def nearest(self, cells, walls):
        cells = np.ascontiguousarray(cells, dtype=np.float64)
        walls = np.ascontiguousarray(walls, dtype=np.float64)
        dist = np.empty(len(cells))
        self.api.check(self.api.nearest_wall_distance(
            self.ctx, len(cells), cells.ctypes.data_as(abi.c_dp), len(walls),
            walls.ctypes.data_as(abi.c_dp), dist.ctypes.data_as(abi.c_dp)),
            "nearest_wall_distance")
        return dist


class Solver:
    def __init__(self, api, case, device=0, rank=0, stream=None, exchange=None,
                 rccl=None):
        """exchange: a DistExchange-like object (multi-process, host buffers);
        rccl: (id128 bytes, nranks, rank) for the library's RCCL transport.  With
        either, iterate() handles connections to other ranks and returns the
        globally reduced norms."""
        self.api, self.case, self.rank = api, case, rank
        self._spectra_book = {}      # gb -> the plan the library holds (spectra_plan)
        self.ctx = C.c_void_p()
        api.check(api.ctx_create(device, rank, C.byref(self.ctx)), "ctx_create")
        if stream is not None:
            api.check(api.ctx_set_stream(self.ctx, C.c_void_p(stream)),
                      "ctx_set_stream")
        self._exchange = exchange
        if exchange is not None:
            api.check(api.set_exchange(self.ctx, C.byref(exchange.struct)), "set_exchange")
        if rccl is not None:
            self._rccl_id = C.create_string_buffer(bytes(rccl[0]), 128)
            api.check(api.rccl_exchange_create(self.ctx, self._rccl_id, rccl[1], rccl[2]),
                      "rccl_exchange_create")
        self.cfg = _b.config_struct(case)
        api.check(api.config_set(self.ctx, C.byref(self.cfg)), "config_set")
        self._keep = []
        self.block_ids = {}
        for gb, blk in enumerate(case.blocks):
            if blk.rank != rank:
                continue
            g = blk.geom
            bg = abi.BlockGeom()
            bg.ni, bg.nj, bg.nk, bg.ng = g.ni, g.nj, g.nk, g.ng
            bg.parent_block, bg.global_pos = blk.parent, blk.global_pos
            if isinstance(g, _geo.NodeGeometry):
                # the nodes alone: the library forms the geometry on the device
                arrs = dict(nodes=g.nodes)
            else:
                arrs = dict(farea_i=g.farea["i"].a, farea_j=g.farea["j"].a,
                            farea_k=g.farea["k"].a, vol=g.vol.a, center=g.center.a,
                            width_i=g.width["i"].a, width_j=g.width["j"].a,
                            width_k=g.width["k"].a, wall_dist=g.wall_dist.a)
            for name, a in arrs.items():
                a = np.ascontiguousarray(a, dtype=np.float64)
                self._keep.append(a)
                setattr(bg, name, a.ctypes.data_as(abi.c_dp))
            bid = C.c_int(-1)
            api.check(api.block_create(self.ctx, C.byref(bg), C.byref(bid)),
                      "block_create")
            self.block_ids[gb] = bid.value
            surfs = _b.surface_structs(case, gb)
            api.check(api.block_set_bcs(self.ctx, bid.value, len(surfs), surfs),
                      "block_set_bcs")
        self.conn_ids = []
        for conn in case.connections:
            if rank not in conn.rank:
                self.conn_ids.append(-1)
                continue
            cs = _b.connection_struct(conn)
            for side in range(2):
                if conn.rank[side] == rank:
                    cs.local_block[side] = self.block_ids[conn.block[side]]
            cid = C.c_int(-1)
            api.check(api.conn_create(self.ctx, C.byref(cs), C.byref(cid)),
                      "conn_create")
            self.conn_ids.append(cid.value)
        api.check(api.setup_finalize(self.ctx), "setup_finalize")
        for gb, bid in self.block_ids.items():
            st = case.blocks[gb].state
            if isinstance(st, _b.StateRecipe):      # build_case(initial="device")
                self.realise(gb, st)
            else:
                self.upload("state", gb, st)
        self.l2_first = None
        self.history = []

    # ------------------------------------------------------------------
    def close(self):
        if self.ctx:
            self.api.ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shape(self, field, gb):
        g = self.case.blocks[gb].geom
        ng = g.ng
        n_eq = self.cfg.n_eq
        ghost = field in ("state", "update", "temperature", "viscosity")
        comps = n_eq if field in ("state", "residual", "cons_n", "update",
                                  "cons_nm1") else \
            9 if field == "vel_grad" else \
            3 if field in ("temp_grad", "dens_grad", "press_grad") else 1
        pad = 2 * ng if ghost else 0
        return (g.nk + pad, g.nj + pad, g.ni + pad, comps)

    def upload(self, field, gb, arr):
        a = np.ascontiguousarray(arr, dtype=np.float64)
        assert a.shape == self._shape(field, gb), (a.shape, self._shape(field, gb))
        if field == "state":
            rc = self.api.state_upload(self.ctx, self.block_ids[gb],
                                       a.ctypes.data_as(abi.c_dp))
        else:
            rc = self.api.field_upload(self.ctx, self.block_ids[gb],
                                       abi.FIELD[field],
                                       a.ctypes.data_as(abi.c_dp))
        self.api.check(rc, "upload")

    def _pack(self, gb, ids, shape):
        """agx_output_pack of block gb with these ids (of one range) into a new array."""
        ids = (C.c_int32 * len(ids))(*ids)
        out = np.empty(shape)
        self.api.check(self.api.output_pack(self.ctx, self.block_ids[gb], len(ids), ids,
                                            out.ctypes.data_as(abi.c_dp)), "output_pack")
        return out

    @staticmethod
    def _per_surface(surfs, names, out):
        """A [nvar, total] wall payload as {name: [one array per surface, in its shape]}."""
        res = {}
        for q, name in enumerate(names):
            off, rows = 0, []
            for s in surfs:
                cnt = int(np.prod(s["shape"]))
                rows.append(out[q, off:off + cnt].reshape(s["shape"]).copy())
                off += cnt
            res[name] = rows
        return res

    def output_pack(self, gb, names):
        """WriteFunFile's variables of block gb (reference names, abi.OUT), packed by the
        library: [nvar, nk, nj, ni], dimensional."""
        ni, nj, nk = self.case.blocks[gb].geom.n
        return self._pack(gb, [abi.OUT[n] for n in names], (len(names), nk, nj, ni))

    def node_pack(self, gb, names):
        """WriteNodeFun's variables of block gb (reference names, abi.NODE_OUT), converted to
        the block's nodes and packed by the library: [nvar, nk + 1, nj + 1, ni + 1],
        dimensional."""
        ni, nj, nk = self.case.blocks[gb].geom.n
        return self._pack(gb, [abi.NODE_OUT[n] for n in names],
                          (len(names), nk + 1, nj + 1, ni + 1))

    def wall_surfaces(self, gb):
        """The viscousWall surfaces of block gb in the order of the wall payload (the order
        the library got them in, which is the order of the reference's wallData_): per surface
        its side (surface type 1..6), its index range and the shape (nk, nj, ni) of its faces."""
        out = []
        for s in self.case.blocks[gb].surfaces:
            if s.bc_type != "viscousWall":
                continue
            side = s.surface_type()
            d = (side - 1) // 2
            n = [s.imax - s.imin, s.jmax - s.jmin, s.kmax - s.kmin]
            n[d] = 1
            out.append(dict(side=side, tag=s.tag, range=(s.imin, s.imax, s.jmin, s.jmax,
                                                         s.kmin, s.kmax),
                            shape=(n[2], n[1], n[0])))
        return out

    def wall_pack(self, gb, names):
        """WriteWallFun's variables of block gb (reference names, abi.WALL_OUT), packed by the
        library: {name: [one array per wall surface, shaped (nk, nj, ni) of its range]},
        dimensional.  A name given twice keeps its last row."""
        surfs = self.wall_surfaces(gb)
        total = sum(int(np.prod(s["shape"])) for s in surfs)
        out = self._pack(gb, [abi.WALL_OUT[n] for n in names], (len(names), total))
        return self._per_surface(surfs, names, out)

    def load_surfaces(self, gb):
        """The load surfaces of block gb -- viscousWall and slipWall -- in the order of the
        load payload (the order the library got them in): like wall_surfaces, with each
        surface's bc_type."""
        out = []
        for s in self.case.blocks[gb].surfaces:
            if s.bc_type not in ("viscousWall", "slipWall"):
                continue
            side = s.surface_type()
            d = (side - 1) // 2
            n = [s.imax - s.imin, s.jmax - s.jmin, s.kmax - s.kmin]
            n[d] = 1
            out.append(dict(side=side, tag=s.tag, bc_type=s.bc_type,
                            range=(s.imin, s.imax, s.jmin, s.jmax, s.kmin, s.kmax),
                            shape=(n[2], n[1], n[0])))
        return out

    def load_names(self, gb):
        """The load variables block gb can give: all of abi.LOAD_OUT for a block built from its
        nodes, without the moments for one built from host arrays (no face centres)."""
        node_built = isinstance(self.case.blocks[gb].geom, _geo.NodeGeometry)
        return [n for n in abi.LOAD_OUT if node_built or n not in abi.LOAD_MOMENTS]

    def wall_loads(self, gb, names=None, about=None):
        """The integrated loads of block gb's load surfaces (abi.LOAD_OUT), summed by the
        library: {name: ndarray[nsurf]}, dimensional, on the wall (the normal points into the
        fluid).  names: default load_names(gb).  about: a reference point (x, y, z) in metres;
        the moments come back about it, M - about x F (the forces are fetched if the call
        does not name them)."""
        names = list(self.load_names(gb) if names is None else names)
        ask = list(names)
        if about is not None:
            for kind in ("pressure", "viscous"):
                if any(n.startswith(kind + "Moment") for n in names):
                    ask += [f"{kind}Force_{c}" for c in "xyz" if f"{kind}Force_{c}" not in ask]
        nsurf = len(self.load_surfaces(gb))
        out = self._pack(gb, [abi.LOAD_OUT[n] for n in ask], (len(ask), max(nsurf, 1)))
        got = {n: out[q, :nsurf].copy() for q, n in enumerate(ask)}
        if about is not None:
            r = [float(x) for x in about]
            for kind in ("pressure", "viscous"):
                f = [got.get(f"{kind}Force_{c}") for c in "xyz"]
                for c, name in enumerate(f"{kind}Moment_{x}" for x in "xyz"):
                    if name in names:
                        c1, c2 = (c + 1) % 3, (c + 2) % 3
                        got[name] = got[name] - (r[c1] * f[c2] - r[c2] * f[c1])
        return {n: got[n] for n in names}

    def total_loads(self, tags=None, about=None):
        """The loads of this rank's blocks summed over their load surfaces, in the fixed order
        (block, surface): {name: float}.  tags: only surfaces whose BC tag is listed.  The
        names are those every block with a load surface can give."""
        blocks = [gb for gb in sorted(self.block_ids) if self.load_surfaces(gb)]
        names = [n for n in abi.LOAD_OUT if all(n in self.load_names(gb) for gb in blocks)]
        total = {n: 0.0 for n in names}
        for gb in blocks:
            got = self.wall_loads(gb, names, about=about)
            for q, s in enumerate(self.load_surfaces(gb)):
                if tags is None or s["tag"] in tags:
                    for n in names:
                        total[n] += float(got[n][q])
        return total

    # -- boundary fluxes and the block balance ----------------------------------------------
    def _remote_surface(self, gb, s):
        """Is surface s of block gb (part of) a connection whose partner is on another rank?"""
        if s.bc_type not in ("interblock", "periodic"):
            return False
        side = s.surface_type()
        d3 = (side - 1) // 2
        d1, d2 = (d3 + 1) % 3, (d3 + 2) % 3
        lo, hi = (s.imin, s.jmin, s.kmin), (s.imax, s.jmax, s.kmax)
        for conn in self.case.connections:
            if conn.rank[0] == conn.rank[1]:
                continue
            for m in range(2):
                if conn.rank[m] == self.rank and conn.block[m] == gb and \
                        conn.boundary[m] == side and conn.d1s[m] < hi[d1] and \
                        conn.d1e[m] > lo[d1] and conn.d2s[m] < hi[d2] and conn.d2e[m] > lo[d2]:
                    return True
        return False

    def flux_surfaces(self, gb):
        """The flux surfaces of block gb in the order of the flux payload: every surface the
        library got, in that order, of every BC type -- local interblock / periodic connections
        included, connections to other ranks left out (their ghost cells are current only
        between exchanges).  Per surface its side (surface type 1..6), BC type, tag, index
        range and the shape (nk, nj, ni) of its faces."""
        out = []
        for s in self.case.blocks[gb].surfaces:
            if self._remote_surface(gb, s):
                continue
            side = s.surface_type()
            d = (side - 1) // 2
            n = [s.imax - s.imin, s.jmax - s.jmin, s.kmax - s.kmin]
            n[d] = 1
            out.append(dict(side=side, tag=s.tag, bc_type=s.bc_type,
                            range=(s.imin, s.imax, s.jmin, s.jmax, s.kmin, s.kmax),
                            shape=(n[2], n[1], n[0])))
        return out

    def flux_names(self, out=None):
        """The names of abi.FLUX_OUT (or of `out`, e.g. abi.BUDGET_OUT) this library gives: the
        5-equation libraries refuse the tke and sdr ids."""
        out = abi.FLUX_OUT if out is None else out
        drop = () if self.cfg.n_eq == 7 else ("_tke", "_sdr")
        return [n for n in out if not n.endswith(drop)]

    def surface_fluxes(self, gb, names=None):
        """What crosses each flux surface of block gb (abi.FLUX_OUT), summed by the library
        from the face fluxes the residual pass takes: {name: ndarray[nsurf]}, SI, positive
        out of the block; inviscid_e + viscous_e is the net outward flux of equation e."""
        names = list(self.flux_names() if names is None else names)
        nsurf = len(self.flux_surfaces(gb))
        out = self._pack(gb, [abi.FLUX_OUT[n] for n in names], (len(names), max(nsurf, 1)))
        return {n: out[q, :nsurf].copy() for q, n in enumerate(names)}

    def block_budget(self, gb, names=None):
        """The balance of block gb (abi.BUDGET_OUT) over its physical cells: {name: float}, SI
        -- the volume, the conserved totals of the state now and the sums of the residual as
        the last residual pass left it."""
        names = list(self.flux_names(abi.BUDGET_OUT) if names is None else names)
        out = self._pack(gb, [abi.BUDGET_OUT[n] for n in names], len(names))
        return {n: float(out[q]) for q, n in enumerate(names)}

    def flux_balance(self, gb):
        """{equation: (residual sum, flux sum)} of block gb: the sum of the residual over the
        physical cells against the net outward flux through all flux surfaces, added in
        surface order.  Equal to rounding right after a residual wherever the equation has no
        source term and the rank holds all of the block's surfaces; after an update the
        residual belongs to the state before it."""
        eqs = abi.EQUATIONS[:self.cfg.n_eq]
        flux = self.surface_fluxes(gb, [f"{kind}_{e}" for e in eqs
                                        for kind in ("inviscid", "viscous")])
        resid = self.block_budget(gb, [f"residual_{e}" for e in eqs])
        out = {}
        for e in eqs:
            total = 0.0
            for a, b in zip(flux[f"inviscid_{e}"], flux[f"viscous_{e}"]):
                total += float(a) + float(b)
            out[e] = (resid[f"residual_{e}"], total)
        return out

    # -- time statistics, kept by the library on the device -----------------------------
    def _stat_dims(self, gb):
        """(cell planes, wall values per face, cells, wall faces) of block gb's accumulators."""
        cfg = self.cfg
        eddy = cfg.n_eq == 7 or cfg.equation_set == abi.EQN["largeEddySimulation"]
        planes = 9 + int(eddy) + (2 if cfg.n_eq == 7 else 0) + abi.STAT_SECOND
        faces = sum(int(np.prod(s["shape"])) for s in self.wall_surfaces(gb))
        wall = abi.STAT_WALL_VALUES if cfg.is_viscous and faces else 0
        ni, nj, nk = self.case.blocks[gb].geom.n
        return planes, wall, ni * nj * nk, faces

    def _stat_weight(self, gb, w):
        one = np.array([w], dtype=np.float64)
        self.api.check(self.api.field_upload(self.ctx, self.block_ids[gb],
                                             abi.FIELD["stat_sample"],
                                             one.ctypes.data_as(abi.c_dp)), "stats_sample")
        # (W, samples) as the library keeps them: the same two additions in float64
        book = self.__dict__.setdefault("_stat_book", {})
        if w == 0.0:
            book.pop(gb, None)
        else:
            big_w, n = book.get(gb, (0.0, 0))
            book[gb] = (big_w + w, n + 1)

    def stats_sample(self, weight=1.0):
        """The current state of every block of this rank enters its running statistics with
        this weight (means and second central moments per cell and per viscousWall face, West's
        recurrence; AGX_FIELD_STAT_SAMPLE).  Call it after a time step has converged.  A weight
        of 0 discards the statistics; the library refuses a negative or non-finite one.
        Block by block, not all or nothing: a block with viscousWall faces refuses the sample
        between phase_bc_faces and phase_residual, a block without takes it there, so a call
        that raises has sampled the blocks before the refusing one (stats_weight tells).  Call
        it between time steps, where every block is legal.  Each block with wall faces refills
        the ghost cells of the whole context before it evaluates its faces."""
        for gb in sorted(self.block_ids):
            self._stat_weight(gb, float(weight))

    def stats_reset(self):
        """Discard the statistics of every block of this rank; the next sample starts anew."""
        for gb in sorted(self.block_ids):
            self._stat_weight(gb, 0.0)

    def stats_download(self, gb):
        """The raw accumulators of block gb (AGX_FIELD_STAT_ACCUM): a flat array of
        {planes, wall values, W, samples}, the cell planes, the wall rows -- what
        stats_upload takes to go on with the average in another run."""
        planes, wall, ncell, faces = self._stat_dims(gb)
        out = np.empty(4 + planes * ncell + wall * faces)
        self.api.check(self.api.field_download(self.ctx, self.block_ids[gb],
                                               abi.FIELD["stat_accum"],
                                               out.ctypes.data_as(abi.c_dp)), "stats_download")
        self.__dict__.setdefault("_stat_book", {})[gb] = (float(out[2]), int(out[3]))
        return out

    def stats_upload(self, gb, payload):
        a = np.ascontiguousarray(payload, dtype=np.float64)
        planes, wall, ncell, faces = self._stat_dims(gb)
        # (the header's two counts are the library's to judge; the length must fit them)
        assert a.ndim == 1 and a.size >= 4 and \
            a.size == 4 + int(a[0]) * ncell + int(a[1]) * faces, a.shape
        self.api.check(self.api.field_upload(self.ctx, self.block_ids[gb],
                                             abi.FIELD["stat_accum"],
                                             a.ctypes.data_as(abi.c_dp)), "stats_upload")
        self.__dict__.setdefault("_stat_book", {})[gb] = (float(a[2]), int(a[3]))

    def stats_weight(self, gb):
        """(sum of weights, samples) of block gb's statistics.  Every sample, reset, upload and
        download of this Solver goes through the methods above, which keep the pair as the
        library does (the same float64 additions; an upload or a download sets it from the
        payload's header), so no plane moves.  A block this Solver has no record of is asked
        with one download of its payload (2.4 GB at 256^3), which the library refuses by name
        before the first sample."""
        book = self.__dict__.setdefault("_stat_book", {})
        if gb not in book:
            self.stats_download(gb)
        return book[gb]

    def stats_pack(self, gb, names):
        """Time statistics of block gb's cells (abi.STAT_OUT), shaped like output_pack:
        [nvar, nk, nj, ni], dimensional."""
        ni, nj, nk = self.case.blocks[gb].geom.n
        return self._pack(gb, [abi.STAT_OUT[n] for n in names], (len(names), nk, nj, ni))

    def stats_collapse(self, gb, names, over):
        """Time statistics of block gb's cells (abi.STAT_OUT and "volume") pooled, volume
        weighted, over the index directions of `over` -- a string out of "i", "j", "k", e.g.
        "ik" -- by the library (AGX_CSTAT_BASE): [nvar, *remaining extents in (k, j, i) order],
        dimensional; over="ijk" gives [nvar].  A mean is the pooled mean, a second moment the
        co-moment about the space-time mean of the bin.  pool_bins joins blocks and ranks."""
        mask = abi.cstat_mask(over)
        ni, nj, nk = self.case.blocks[gb].geom.n
        rest = tuple(n for bit, n in ((4, nk), (2, nj), (1, ni)) if not mask & bit)
        return self._pack(gb, [abi.cstat_id(mask, n) for n in names], (len(names),) + rest)

    def wall_stats_pack(self, gb, names):
        """Time statistics of block gb's viscousWall faces (abi.WALL_STAT_OUT), shaped like
        wall_pack: {name: [one array per wall surface]}, dimensional."""
        surfs = self.wall_surfaces(gb)
        total = sum(int(np.prod(s["shape"])) for s in surfs)
        out = self._pack(gb, [abi.WALL_STAT_OUT[n] for n in names],
                         (len(names), max(total, 1)))
        return self._per_surface(surfs, names, out)

    # -- time series at chosen cells and wall faces, recorded on the device ----------------
    def _series_up(self, gb, field, payload, what):
        a = np.ascontiguousarray(payload, dtype=np.float64)
        self.api.check(self.api.field_upload(self.ctx, self.block_ids[gb], abi.FIELD[field],
                                             a.ctypes.data_as(abi.c_dp)), what)

    def _series_down(self, gb, field, size, what):
        out = np.empty(size)
        self.api.check(self.api.field_download(self.ctx, self.block_ids[gb], abi.FIELD[field],
                                               out.ctypes.data_as(abi.c_dp)), what)
        return out

    def series_plan(self, gb, names, points, capacity, kind="cells"):
        """Plan the time series of block gb (AGX_FIELD_SERIES_PLAN): the variables `names`
        (abi.OUT for kind "cells", abi.WALL_OUT for kind "wall") at `points` -- [P, 3] cells
        (i, j, k), or [P] indices into the wall payload in the order of wall_pack's rows
        concatenated over wall_surfaces(gb).  Replaces the block's plan, discards its rows and
        allocates a ring of `capacity` rows on the device; no points discards the plan."""
        payload = abi.series_plan(names, points, capacity, kind)
        self._series_up(gb, "series_plan", payload, "series_plan")
        book = self.__dict__.setdefault("_series_book", {})
        if int(payload[1]) == 0:
            book.pop(gb, None)
        else:
            # [P, V, capacity, rows]: what sizes a collect, kept as the library keeps it
            book[gb] = [int(payload[1]), len(names), int(capacity), 0]

    def series_sample(self, t):
        """Append one row -- t and the planned variables at the planned points, exactly what
        output_pack / wall_pack hold there now -- to the record of every block of this rank
        that has a plan, in ascending gb (AGX_FIELD_SERIES_SAMPLE).  One kernel per block on
        the context's stream: no synchronisation, no copy, no allocation.  A full record
        refuses: collect (series_rows) and drop (series_drop) first.
        Block by block, not all or nothing: a plan with gradient names and every wall plan
        refuse between phase_bc_faces and phase_residual, a plan of plain cell variables
        samples there, so a call that raises has sampled the blocks before the refusing one.
        Call it between time steps, where every plan is legal."""
        one = np.array([float(t)])
        for gb in sorted(self.__dict__.get("_series_book", {})):
            self._series_up(gb, "series_sample", one, "series_sample")
            self._series_book[gb][3] += 1

    def series_rows(self, gb):
        """The record of block gb, oldest row first: (t[rows], values[rows, V, P]), dimensional
        (AGX_FIELD_SERIES_ROWS; synchronises, leaves the record as it is)."""
        npts, nvar, cap, _ = self.__dict__.get("_series_book", {}).get(gb, (0, 0, 0, 0))
        out = self._series_down(gb, "series_rows", abi.series_rows_size(npts, nvar, cap),
                                "series_rows")
        return abi.series_rows_split(out)

    def series_drop(self, gb, n=None):
        """Drop the oldest n rows of block gb's record (all of them by default), making room
        for as many samples: the record is a ring and never reallocates."""
        entry = self.__dict__.get("_series_book", {}).get(gb)
        if n is None:
            n = entry[3] if entry else 0
        self._series_up(gb, "series_rows", np.array([float(n)]), "series_drop")
        if entry:
            entry[3] -= int(n)

    def series_clear(self):
        """Discard the plan and the record of every block of this rank."""
        for gb in sorted(self.__dict__.get("_series_book", {})):
            self.series_plan(gb, [], [], 1)

    def series_locate(self, points):
        """For each of points[P, 3] (in the units of the "center" field) the physical cell of
        this rank's blocks whose centre is nearest, searched on the device
        (AGX_FIELD_SERIES_LOCATE, every block of the rank): [P, 5] = (gb, i, j, k, d2).  Among
        equally near cells of a block the lowest (k nj + j) ni + i wins, among blocks at equal
        d2 the lowest gb.  pool_series joins the results of ranks."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        payload = np.concatenate([[float(len(pts))], pts.ravel()])
        parts = []
        for gb in sorted(self.block_ids):
            self._series_up(gb, "series_locate", payload, "series_locate")
            got = self._series_down(gb, "series_locate", 4 * len(pts), "series_locate")
            parts.append(np.column_stack([np.full(len(pts), float(gb)), got.reshape(-1, 4)]))
        return pool_series(parts)

    def series_plan_located(self, where, names, capacity):
        """Plan every block of this rank for the points of `where` ([P, 5] of series_locate or
        pool_series) that lie in it.  Returns {gb: indices into `where` of its points}, the
        order of the block's points in its rows."""
        where = np.asarray(where)
        mine = {}
        for gb in sorted(self.block_ids):
            at = np.flatnonzero(where[:, 0] == gb)
            if at.size:
                self.series_plan(gb, names, where[at, 1:4], capacity)
                mine[gb] = at
        return mine

    # -- spectra along homogeneous directions, accumulated on the device ----------------------
    def spectra_plan(self, gb, names, pairs=(), along="i", over=""):
        """Plan the spectra of block gb (AGX_FIELD_SPECTRA_PLAN): the auto-spectra of `names`
        (out of abi.SPECTRA_NAMES, at most 6) and the co-spectra of `pairs` (two names, or two
        indices into names) along index direction `along`, the lines pooled with equal weights
        over the directions of `over` (a string out of the other two).  Replaces the block's
        plan, discards its accumulators and allocates; no names frees everything."""
        payload = abi.spectra_plan(names, pairs, along, over)
        self._series_up(gb, "spectra_plan", payload, "spectra_plan")
        book = self._spectra_book
        if not len(names):
            book.pop(gb, None)
            return
        ni, nj, nk = self.case.blocks[gb].geom.n
        rest, nmode = abi.spectra_shape((ni, nj, nk), along, over)
        lines = int(np.prod([(ni, nj, nk)["ijk".index(d)] for d in over] or [1]))
        book[gb] = {"payload": payload, "rest": rest, "nmode": nmode, "lines": lines,
                    "n": (ni, nj, nk)["ijk".index(along)]}

    def spectra_sample(self, weight=1.0):
        """One sample of the state the device holds now into the spectra of every block of this
        rank that has a plan, in ascending gb (AGX_FIELD_SPECTRA_SAMPLE): two kernels per block
        on the context's stream, no synchronisation, no copy, no allocation.  Reads physical
        cells only: legal at every position of the phase API."""
        one = np.array([float(weight)])
        for gb in sorted(self._spectra_book):
            self._series_up(gb, "spectra_sample", one, "spectra_sample")

    def spectra_reset(self):
        """Discard the accumulated spectra of every planned block; the plans stay."""
        self.spectra_sample(0.0)

    def spectra_clear(self):
        """Discard the plan and the spectra of every block of this rank."""
        for gb in sorted(self._spectra_book):
            self.spectra_plan(gb, [])

    def _spectra_entry(self, gb):
        entry = self._spectra_book.get(gb)
        # (a block without a plan: the library refuses by name; one double is enough)
        return entry or {"payload": np.zeros(4), "rest": (), "nmode": 1, "lines": 1, "n": 2}

    def spectra_download(self, gb):
        """The raw payload of block gb's spectra (AGX_FIELD_SPECTRA_ACCUM): the plan,
        {W, samples, nbin, nmode} and the nondimensional S; abi.spectra_accum_split reads it."""
        e = self._spectra_entry(gb)
        nvar, npair = int(e["payload"][2]), int(e["payload"][3])
        nbin = int(np.prod(e["rest"] or (1,)))
        return self._series_down(gb, "spectra_accum",
                                 abi.spectra_accum_size(nvar, npair, nbin, e["nmode"]),
                                 "spectra_download")

    def spectra_upload(self, gb, payload):
        """Carry an average on: the payload of spectra_download into block gb, which must hold
        the same plan (refused by name otherwise)."""
        self._series_up(gb, "spectra_accum", payload, "spectra_upload")

    def spectra(self, gb):
        """The spectra of block gb (AGX_FIELD_SPECTRA_VALUES), dimensional:
        (values[nspec, *remaining extents in (k, j, i) order, nmode], W, samples); the spectra
        are the variables in plan order, then the pairs."""
        e = self._spectra_entry(gb)
        nspec = int(e["payload"][2]) + int(e["payload"][3])
        nbin = int(np.prod(e["rest"] or (1,)))
        out = self._series_down(gb, "spectra_values", max(nspec * nbin * e["nmode"], 1),
                                "spectra")
        _, W, samples, _ = abi.spectra_accum_split(self.spectra_download(gb))
        return out.reshape((nspec,) + tuple(e["rest"]) + (e["nmode"],)), W, samples

    def spectra_lines(self, gb):
        """Lines of a bin of block gb's plan (what pool_spectra weighs a part by, with W)."""
        return self._spectra_entry(gb)["lines"]

    def restart_pack(self, gb, which=0):
        """WriteRestart's payload of block gb: [nk, nj, ni, n_eq + 1], dimensional."""
        g = self.case.blocks[gb].geom
        ni, nj, nk = g.n
        out = np.empty((nk, nj, ni, self.cfg.n_eq + 1))
        self.api.check(self.api.restart_pack(self.ctx, self.block_ids[gb], which,
                                             out.ctypes.data_as(abi.c_dp)), "restart_pack")
        return out

    # -- the state a run starts or resumes from, formed by the library ------------------
    def state_fill(self, gb, prim):
        """procBlock::InitializeStates, non-file branch: every physical cell of block gb takes
        the nondimensional primitive prim[n_eq], every ghost cell zero (agx_state_fill)."""
        p = np.ascontiguousarray(prim, dtype=np.float64)
        assert p.shape == (self.cfg.n_eq,), p.shape
        self.api.check(self.api.state_fill(self.ctx, self.block_ids[gb],
                                           p.ctypes.data_as(abi.c_dp)), "state_fill")

    def state_from_cloud(self, gb, pts, st):
        """The file branch: every physical cell takes the state of the nearest of the cloud's
        points (pts[npts, 3], st[npts, n_eq] of builder.cloud_states; among equally near points
        the lowest index), every ghost cell zero.  Returns the reference's maxDist."""
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        st = np.ascontiguousarray(st, dtype=np.float64)
        assert pts.ndim == 2 and pts.shape[1] == 3 and st.shape == (len(pts), self.cfg.n_eq), \
            (pts.shape, st.shape)
        far = C.c_double(0.0)
        self.api.check(self.api.state_from_cloud(
            self.ctx, self.block_ids[gb], len(pts), pts.ctypes.data_as(abi.c_dp),
            st.ctypes.data_as(abi.c_dp), C.byref(far)), "state_from_cloud")
        return far.value

    def restart_unpack(self, gb, payload, which=0):
        """The inverse of restart_pack: a block's restart payload [nk, nj, ni, n_eq + 1],
        nondimensionalised by the library into the state (which = 0, ghost cells zero) or
        consVarsNm1 (which = 1)."""
        g = self.case.blocks[gb].geom
        ni, nj, nk = g.n
        a = np.ascontiguousarray(payload, dtype=np.float64)
        assert a.shape == (nk, nj, ni, self.cfg.n_eq + 1), a.shape
        self.api.check(self.api.restart_unpack(self.ctx, self.block_ids[gb], which,
                                               a.ctypes.data_as(abi.c_dp)), "restart_unpack")

    def realise(self, gb, recipe):
        """A builder.StateRecipe into the state of block gb, on the device."""
        if recipe.kind == "uniform":
            return self.state_fill(gb, recipe.prim)
        if recipe.kind == "cloud":
            return self.state_from_cloud(gb, recipe.pts, recipe.st)
        raise ValueError(f"state recipe of kind {recipe.kind!r}: 'uniform' or 'cloud'")

    def download(self, field, gb):
        if field in abi.GEOM_FIELDS:
            return self.geometry(field, gb)
        out = np.empty(self._shape(field, gb))
        self.api.check(self.api.field_download(
            self.ctx, self.block_ids[gb], abi.FIELD[field],
            out.ctypes.data_as(abi.c_dp)), "field_download")
        return out

    def geometry(self, name, gb):
        """One of the geometry arrays of block gb as the device holds it (abi.GEOM_FIELDS:
        volume, center, farea_i/j/k, width_i/j/k, wall_dist), in the host layout
        agx_block_geom documents, ghost cells included.  For a block created from its nodes
        this is the only place its centres or wall distance can be had."""
        comps, face = abi.GEOM_FIELDS[name]
        g = self.case.blocks[gb].geom
        pad = 2 * g.ng
        out = np.empty((g.nk + pad + (face == "k"), g.nj + pad + (face == "j"),
                        g.ni + pad + (face == "i"), comps))
        self.api.check(self.api.field_download(
            self.ctx, self.block_ids[gb], abi.FIELD[name],
            out.ctypes.data_as(abi.c_dp)), "field_download")
        return out

    # ------------------------------------------------------------------
    def store_time_n(self, nn):
        d = self.case.deck
        if d.need_to_store_time_n():
            also = int(d.is_multilevel_in_time() and nn == 0)
            self.api.check(self.api.store_time_n(self.ctx, also), "store_time_n")

    def iterate(self, mm, cfl):
        n_eq = self.cfg.n_eq
        l2 = np.zeros(n_eq)
        linf = abi.Linf()
        mres = C.c_double(0.0)
        self._check(self.api.iterate(
            self.ctx, mm, cfl, l2.ctypes.data_as(abi.c_dp), C.byref(linf),
            C.byref(mres)), "iterate")
        return l2, linf, mres.value

    def _check(self, rc, what):
        """api.check for a call that runs the exchange: an exception one of its callbacks
        raised (kept in exchange.pending; the library saw a failed operation) is the cause of
        the RuntimeError and named in its text."""
        exc = getattr(self._exchange, "pending", None)
        if exc is not None:
            self._exchange.pending = None
        try:
            self.api.check(rc, what)
        except RuntimeError as err:
            if exc is None:
                raise
            raise RuntimeError(f"{err} [the exchange raised {exc!r}]") from exc

    def normalized(self, l2sq, nn, mm):
        """PrintResiduals (output.cpp:1028-1087) for the single-species case."""
        l2 = np.sqrt(l2sq)                 # residual::SquareRoot (main.cpp:268)
        if nn == 0 and mm == 0:
            self.l2_first = l2.copy()
        elif nn < 5 and mm == 0:
            if l2[0] > self.l2_first[0]:
                self.l2_first[0] = l2[0]
            self.l2_first[1:] = np.maximum(self.l2_first[1:], l2[1:])
        return (l2 + EPS) / (self.l2_first + EPS)

    def step(self, nn):
        d = self.case.deck
        cfl = d.cfl(nn)
        self.store_time_n(nn)
        out = None
        for mm in range(d.nonlinear_iterations):
            l2, linf, mres = self.iterate(mm, cfl)
            total = self.case.total_cells
            mres = math.sqrt(mres / (total * self.cfg.n_eq))   # main.cpp:271
            out = dict(nn=nn, mm=mm, l2=np.sqrt(l2),
                       norm=self.normalized(l2, nn, mm),
                       linf=(linf.linf, linf.block, linf.i, linf.j, linf.k,
                             linf.eqn), matrix=mres)
            self.history.append(out)
        return out

    def run(self, iterations):
        out = None
        for nn in range(iterations):
            out = self.step(nn)
        return out


class PhasedSolver(Solver):
    """One rank of a multi-process run: blocks whose `rank` matches are local,
    connections to other ranks exchange halo slabs between the phases of
    agx_iterate (include/aither_gfx950.h "phases").

    `exchange(items)` is supplied by the caller: items is a list of
    (peer_rank, tag, send_tensor, recv_tensor); it must complete all transfers
    (torch.distributed batch_isend_irecv over RCCL on GPUs, gloo on CPU).
    `alloc(n)` returns a float64 tensor of n elements on the backend's memory
    (torch.cuda for the product library, CPU for the test oracle).
    This is the drop-in replacement of the reference's MPI path
    (multiArray3d.hpp:830-866 SwapSliceParallel, utility.cpp:400-423).
    """

    def __init__(self, api, case, rank, exchange, alloc, device=0, stream=None):
        super().__init__(api, case, device=device, rank=rank, stream=stream)
        self.exchange, self.alloc = exchange, alloc
        self.remote = []
        for n, conn in enumerate(case.connections):
            if rank in conn.rank and conn.rank[0] != conn.rank[1]:
                side = 0 if conn.rank[0] == rank else 1
                cnt = self.api.halo_count(self.ctx, self.conn_ids[n], 0)
                self.remote.append(dict(
                    cid=self.conn_ids[n], tag=n, peer=conn.rank[1 - side],
                    send=self.alloc(cnt), recv=self.alloc(cnt)))

    def _halo(self, what):
        api = self.api
        api.check(api.halo_swap_local(self.ctx, what), "halo_swap_local")
        if not self.remote:
            return
        for r in self.remote:
            api.check(api.halo_pack(self.ctx, r["cid"], what,
                                    C.c_void_p(r["send"].data_ptr())), "halo_pack")
        api.check(api.sync(self.ctx), "sync")
        self.exchange([(r["peer"], r["tag"], r["send"], r["recv"])
                       for r in self.remote])
        for r in self.remote:
            api.check(api.halo_unpack(self.ctx, r["cid"], what,
                                      C.c_void_p(r["recv"].data_ptr())),
                      "halo_unpack")

    def iterate(self, mm, cfl):
        api, ctx, cfg = self.api, self.ctx, self.cfg
        l2 = np.zeros(cfg.n_eq)
        linf = abi.Linf()
        mres = C.c_double(0.0)
        l2p = l2.ctypes.data_as(abi.c_dp)
        api.check(api.phase_bc_faces(ctx), "phase_bc_faces")
        self._halo(abi.HALO_STATE)
        api.check(api.phase_bc_edges(ctx), "phase_bc_edges")
        api.check(api.phase_residual(ctx, mm, cfl), "phase_residual")
        if self.case.deck.is_implicit():
            block = cfg.matrix_solver in (abi.SOLVER["blusgs"], abi.SOLVER["bdplur"])
            if block and cfg.is_viscous:      # gridLevel.cpp:386-388
                self._halo(abi.HALO_VELGRAD_A)
                self._halo(abi.HALO_VELGRAD_B)
            if cfg.n_eq == 7:                 # SwapTurbVars gridLevel.cpp:389-392
                self._halo(abi.HALO_TURB)
            api.check(api.phase_implicit_begin(ctx), "phase_implicit_begin")
            lusgs = cfg.matrix_solver in (abi.SOLVER["lusgs"], abi.SOLVER["blusgs"])
            for s in range(cfg.matrix_sweeps):
                self._halo(abi.HALO_UPDATE)
                api.check(api.phase_relax_forward(ctx, s), "relax_forward")
                if lusgs:
                    self._halo(abi.HALO_UPDATE)
                    api.check(api.phase_relax_backward(ctx, s), "relax_backward")
            self._halo(abi.HALO_UPDATE)
            api.check(api.phase_matrix_residual(ctx, C.byref(mres)),
                      "matrix_residual")
            api.check(api.phase_implicit_update(ctx, mm, l2p, C.byref(linf)),
                      "implicit_update")
        else:
            api.check(api.phase_explicit_update(ctx, mm, l2p, C.byref(linf)),
                      "explicit_update")
        return l2, linf, mres.value


class MultigridSolver:
    """mgSolution with more than one grid level (mgSolution.cpp:160-262) on one rank: a Solver
    (a context of the library) per level and the transfers of aither_amd.case.multigrid between
    them.  levels: (cases, transfers) of multigrid.build_levels, finest first.  The cycle
    (V: 1 coarse visit, W: 2) is host logic over the library's phases and the agx_mg_* calls;
    the same driver runs the product library and the test oracle."""

    def __init__(self, api, cases, transfers, device=0, stream=None, rank=0, exchange=None):
        """rank / exchange: one rank of a multi-process run -- the blocks of every level live
        on the rank of their finest ancestor; exchange() returns a fresh DistExchange-like
        object per level (the levels' connections to other ranks go through the library's
        exchange table, agx_halo_exchange).  The norms a rank gets back are its own."""
        self.api = api
        self.levels = [Solver(api, c, device=device, rank=rank, stream=stream,
                              exchange=exchange() if exchange else None) for c in cases]
        self.transfers = []
        for trs in transfers:
            keep = []
            for t in trs:
                keep.append(dict(
                    tc=np.ascontiguousarray(t.to_coarse, dtype=np.int32),
                    vf=np.ascontiguousarray(t.vol_fac, dtype=np.float64),
                    cf=np.ascontiguousarray(t.coeffs, dtype=np.float64)))
            self.transfers.append(keep)
        deck = cases[0].deck
        self.case, self.cfg = cases[0], self.levels[0].cfg
        self.cycle_index = {"V": 1, "W": 2}[deck.multigrid_cycle]   # input.cpp (mgCycleIndex_)
        self.history = []
        self.l2_first = None

    # -- plumbing ----------------------------------------------------------
    def close(self):
        for s in self.levels:
            s.close()

    @property
    def block_ids(self):
        return self.levels[0].block_ids

    # What a Solver gives and the multigrid driver hands on.  Of the finest level: the time
    # statistics, the time series, the spectra.
    _OF_FINEST = (
        "stats_sample", "stats_reset", "stats_weight", "stats_pack", "stats_collapse",
        "wall_stats_pack", "stats_download", "stats_upload",
        "series_plan", "series_sample", "series_rows", "series_drop", "series_clear",
        "series_locate", "series_plan_located",
        "spectra_plan", "spectra_sample", "spectra", "spectra_download", "spectra_upload",
        "spectra_reset", "spectra_clear", "spectra_lines")
    # Of any level, with level=0 after the Solver's own arguments.
    _OF_LEVEL = ("download", "load_surfaces", "wall_loads", "total_loads", "flux_surfaces",
                 "surface_fluxes", "block_budget")

    def _p(self, a, ctype):
        return a.ctypes.data_as(C.POINTER(ctype))

    def _boundary_and_residual(self, s, mm, cfl):
        api = self.api
        api.check(api.phase_bc_faces(s.ctx), "phase_bc_faces")
        api.check(api.halo_exchange(s.ctx, abi.HALO_STATE), "halo_exchange")
        api.check(api.phase_bc_edges(s.ctx), "phase_bc_edges")
        api.check(api.phase_residual(s.ctx, mm, cfl), "phase_residual")
        # gridLevel::CalcResidual ends with SwapEddyViscAndGradients and, for rans,
        # SwapTurbVars (gridLevel.cpp:386-392); Restriction calls it on the coarse level
        # (:559-563), so every level makes these swaps, as PhasedSolver.iterate does
        cfg = s.cfg
        block = cfg.matrix_solver in (abi.SOLVER["blusgs"], abi.SOLVER["bdplur"])
        if block and cfg.is_viscous:
            api.check(api.halo_exchange(s.ctx, abi.HALO_VELGRAD_A), "halo_exchange")
            api.check(api.halo_exchange(s.ctx, abi.HALO_VELGRAD_B), "halo_exchange")
        if cfg.n_eq == 7:
            api.check(api.halo_exchange(s.ctx, abi.HALO_TURB), "halo_exchange")

    # -- linearSolver::Relax (linearSolver.cpp:430-470, :509-536) ---------------
    def relax(self, lev, sweeps):
        api, s = self.api, self.levels[lev]
        lusgs = s.cfg.matrix_solver in (abi.SOLVER["lusgs"], abi.SOLVER["blusgs"])
        for ii in range(sweeps):
            api.check(api.halo_exchange(s.ctx, abi.HALO_UPDATE), "halo_exchange")
            api.check(api.phase_relax_forward(s.ctx, ii), "relax_forward")
            if lusgs:
                api.check(api.halo_exchange(s.ctx, abi.HALO_UPDATE), "halo_exchange")
                api.check(api.phase_relax_backward(s.ctx, ii), "relax_backward")
        api.check(api.halo_exchange(s.ctx, abi.HALO_UPDATE), "halo_exchange")
        mres = C.c_double(0.0)
        api.check(api.mg_matrix_residual(s.ctx, C.byref(mres)), "mg_matrix_residual")
        return mres.value

    # -- gridLevel::Restriction (gridLevel.cpp:538-595) --------------------------
    def restriction(self, fl, mm, cfl):
        api, f, c = self.api, self.levels[fl], self.levels[fl + 1]
        trs = self.transfers[fl]
        for gb, bid in f.block_ids.items():
            t = trs[gb]
            api.check(api.mg_restrict(f.ctx, c.ctx, bid, 0, self._p(t["tc"], C.c_int32),
                                      self._p(t["vf"], C.c_double)), "mg_restrict state")
            if mm == 0:          # need the solution at time n for the linear solvers
                api.check(api.store_time_n(c.ctx, 0), "store_time_n")
        self._boundary_and_residual(c, mm, cfl)
        api.check(api.mg_invert_diagonal(c.ctx), "mg_invert_diagonal")
        for gb, bid in f.block_ids.items():
            t = trs[gb]
            api.check(api.mg_restrict(f.ctx, c.ctx, bid, 1, self._p(t["tc"], C.c_int32),
                                      self._p(t["vf"], C.c_double)), "mg_restrict update")
        api.check(api.halo_exchange(c.ctx, abi.HALO_UPDATE), "halo_exchange")
        for gb, bid in f.block_ids.items():
            t = trs[gb]
            api.check(api.mg_restrict(f.ctx, c.ctx, bid, 2, self._p(t["tc"], C.c_int32),
                                      None), "mg_restrict forcing")

    # -- mgSolution::CycleAtLevel (mgSolution.cpp:160-205) ------------------------
    def cycle(self, fl, mm, cfl):
        api = self.api
        sweeps_all = self.cfg.matrix_sweeps
        if fl == len(self.levels) - 1:
            return self.relax(fl, sweeps_all)
        sweeps = max(sweeps_all // 2, 1)
        self.relax(fl, sweeps)
        cl = fl + 1
        self.restriction(fl, mm, cfl)
        api.check(api.mg_save_update(self.levels[cl].ctx), "mg_save_update")
        for _ in range(self.cycle_index):
            self.cycle(cl, mm, cfl)
        f, c = self.levels[fl], self.levels[cl]
        for gb, bid in f.block_ids.items():
            t = self.transfers[fl][gb]
            api.check(api.mg_prolong(c.ctx, f.ctx, bid, self._p(t["tc"], C.c_int32),
                                     self._p(t["cf"], C.c_double)), "mg_prolong")
        return self.relax(fl, sweeps)

    # -- mgSolution::Iterate / ImplicitUpdate (mgSolution.cpp:207-262) -------------
    def iterate(self, mm, cfl):
        api, f = self.api, self.levels[0]
        l2 = np.zeros(self.cfg.n_eq)
        linf = abi.Linf()
        self._boundary_and_residual(f, mm, cfl)
        api.check(api.phase_implicit_begin(f.ctx), "phase_implicit_begin")
        mres = self.cycle(0, mm, cfl)
        api.check(api.phase_implicit_update(f.ctx, mm, l2.ctypes.data_as(abi.c_dp),
                                            C.byref(linf)), "implicit_update")
        for s in self.levels[1:]:      # ResetDiagonal on every level (mgSolution.cpp:236-239)
            api.check(api.mg_reset_diagonal(s.ctx), "mg_reset_diagonal")
        return l2, linf, mres

    normalized = Solver.normalized

    def step(self, nn):
        d = self.case.deck
        cfl = d.cfl(nn)
        for s in self.levels:          # mgSolution::StoreOldSolution: every level
            s.store_time_n(nn)
        out = None
        for mm in range(d.nonlinear_iterations):
            l2, linf, mres = self.iterate(mm, cfl)
            total = self.case.total_cells
            mres = math.sqrt(mres / (total * self.cfg.n_eq))
            out = dict(nn=nn, mm=mm, l2=np.sqrt(l2), norm=self.normalized(l2, nn, mm),
                       linf=(linf.linf, linf.block, linf.i, linf.j, linf.k, linf.eqn),
                       matrix=mres)
            self.history.append(out)
        return out

    def run(self, iterations):
        out = None
        for nn in range(iterations):
            out = self.step(nn)
        return out


def _forwarder(name, leveled):
    own = getattr(Solver, name).__code__.co_argcount - 1      # (its arguments, without self)

    def method(self, *args, **kw):
        level = 0
        if leveled and len(args) > own:
            *args, level = args
        elif leveled:
            level = kw.pop("level", 0)
        return getattr(self.levels[level], name)(*args, **kw)
    method.__name__ = name
    method.__doc__ = getattr(Solver, name).__doc__
    return method


for _name in MultigridSolver._OF_FINEST + MultigridSolver._OF_LEVEL:
    setattr(MultigridSolver, _name, _forwarder(_name, _name in MultigridSolver._OF_LEVEL))
