"""A fused-Arnoldi workspace (mpg_arnoldi_create) whose state a test injects
and reads back, so that one phase launch at a time can be compared with its
restatement (tests/arnoldi_ref_np.py). Everything goes through the C ABI:
mpg_memcpy_h2d / d2h at the accessor pointers, every launch through hip.check.

Importing this module needs no GPU: tests/test_arnoldi_ref_cpu.py reads the
classes, the matrix list and ld_of from it.

A HIP runtime error in any copy or launch made through a PhaseWorkspace ends
the whole pytest session (PhaseWorkspace._check): after a fault nothing more
is started on the device. tests/test_neumann_gpu.py::Workspace inherits this."""
import ctypes as C

import numpy as np

MPG_F64, MPG_F32, MPG_F16 = 0, 1, 2
TYPES = {"f64": (np.float64, C.c_double, MPG_F64), "f32": (np.float32, C.c_float, MPG_F32)}  # dtype, ctype, mpg_dtype_t
ORTH = {"cgs": 0, "mgs": 1, "cgsr": 2}
MPG_OK, MPG_ERR_HIP, MPG_ERR_UNSUPPORTED = 0, -1, -5

# (t, accum) of the three accumulation classes the phase kernels are built for
CLASSES = {"f32-acc64": ("f32", 0), "f32-acc32": ("f32", 1), "f64": ("f64", 0)}

MATRICES = {
    "band260": lambda m: m.gen_band(260, 5, 4, seed=7),    # two live waves, the second with 4 rows
    "band4099": lambda m: m.gen_band(4099, 5, 4, seed=7),  # n mod 4 = 3, one workgroup
    "band4100": lambda m: m.gen_band(4100, 5, 4, seed=7),  # a second workgroup with one quad
    "band8196": lambda m: m.gen_band(8196, 5, 4, seed=7),  # (step_dots needs n mod 4 = 0)
    "band8197": lambda m: m.gen_band(8197, 5, 4, seed=7),  # three workgroups plus one tail row
    "lap12": lambda m: m.gen_laplace3d(12),
    "stencil5": lambda m: m.gen_stencil27(5),
}


# ---------------------------------------------------------------- the variants' matrices (seeded, hand-built)
FAR = 32_900            # far33k's far columns: r +- FAR, beyond the int16 slice-relative form's +-32767
FAR66_ROW, FAR66 = 33_024, 33_000  # far66k: element 0 of row FAR66_ROW is r - FAR66, of the next row r + FAR66
RANK_SPLITS = {"band-ranks": [0, 4099, 8198, 12297], "band-stiff-ranks": [0, 4099, 8198, 12297],
               "stencil-ranks": [0, 324, 648]}


def _csr_of(mpg, n, rows, cols, vals):
    import scipy.sparse as sp

    M = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    M.sort_indices()
    return mpg.Csr(n, n, M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64))


def _tridiag(n, seed):
    """(rows, cols, vals) of a tridiagonal matrix: diagonal uniform in [3, 5], off-diagonals in [-1, -0.5]."""
    rng = np.random.default_rng(seed)
    r = np.arange(n)
    rows = np.concatenate([r, r[1:], r[:-1]])
    cols = np.concatenate([r, r[1:] - 1, r[:-1] + 1])
    vals = np.concatenate([rng.uniform(3.0, 5.0, n), rng.uniform(-1.0, -0.5, 2 * (n - 1))])
    return rows, cols, vals, rng


def gen_far33k(mpg, n=33_280):
    """Tridiagonal plus entries at column r +- FAR wherever that is in range:
    col - (first row of the slice) leaves +-32767 (the stepped int16 form), and
    no (step, element) position of a slice spreads beyond 65,534 (no slice is
    summed from the sub-CSR)."""
    rows, cols, vals, rng = _tridiag(n, 33)
    r = np.arange(n)
    lo, hi = r[r - FAR >= 0], r[r + FAR < n]
    rows = np.concatenate([rows, lo, hi])
    cols = np.concatenate([cols, lo - FAR, hi + FAR])
    vals = np.concatenate([vals, rng.uniform(0.25, 0.75, len(lo) + len(hi))])
    return _csr_of(mpg, n, rows, cols, vals)


def gen_far66k(mpg, n=66_048):
    """Tridiagonal; row FAR66_ROW also reads column r - FAR66 (its element 0),
    and the next row holds only column r + FAR66 (its element 0): that slice's
    element 0 spreads over 66,000 and the slice is summed from the sub-CSR
    (tests/test_sell_stepped_gpu.py::_far, shrunk)."""
    rows, cols, vals, rng = _tridiag(n, 66)
    keep = rows != FAR66_ROW + 1
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    rows = np.concatenate([rows, [FAR66_ROW, FAR66_ROW + 1]])
    cols = np.concatenate([cols, [FAR66_ROW - FAR66, FAR66_ROW + 1 + FAR66]])
    vals = np.concatenate([vals, [0.25, 0.5]])
    return _csr_of(mpg, n, rows, cols, vals)


def gen_band_stiff(mpg, n=4099):
    """gen_band(n) with every 7th row times 2^20 and every 11th row times 2^-12:
    rows that mpg_csr_half_values scales down, scales up and leaves alone share
    64-row slices."""
    A = mpg.gen_band(n, 5, 4, seed=7)
    r = np.arange(A.nrows)
    f = np.where(r % 7 == 0, 2.0 ** 20, 1.0) * np.where(r % 11 == 0, 2.0 ** -12, 1.0)
    return mpg.Csr(A.nrows, A.ncols, A.rowptr, A.col, A.val * np.repeat(f, np.diff(A.rowptr)))


def gen_stencil_rows(mpg, nx=5):
    """gen_stencil27(nx) with row i scaled by a factor in [0.5, 2] of its own: the 3 x 3 diagonal blocks, which
    the stencil has symmetric, lose their symmetry, and so do their inverses (block Jacobi read transposed)."""
    A = mpg.gen_stencil27(nx)
    f = np.random.default_rng(27).uniform(0.5, 2.0, A.nrows)
    return mpg.Csr(A.nrows, A.ncols, A.rowptr, A.col, A.val * np.repeat(f, np.diff(A.rowptr)))


MATRICES.update({
    "stencil5-rows": gen_stencil_rows,
    "far33k": gen_far33k, "far66k": gen_far66k, "band-stiff": gen_band_stiff,
    "band-stiff8197": lambda m: gen_band_stiff(m, 8197),          # every slice as wide: two slices per wave
    "band-stiff-ranks": lambda m: gen_band_stiff(m, 3 * 4099),    # (RANK_SPLITS)
    "band-ranks": lambda m: m.gen_band(3 * 4099, 5, 4, seed=7),  # split into three row blocks (RANK_SPLITS)
    "stencil-ranks": lambda m: m.gen_stencil27(6),               # two row blocks of 108 nodes: a gathered halo
})


class RankBlock:
    """Rows row_starts[rank] .. row_starts[rank + 1] of A as the row-partitioned
    engine holds them: local column ids from HaloPlan.local_cols() (lower
    ranks' halo rows at [-n_front, 0), higher ranks' at [n, n_ext)).
    .A: the local matrix (ncols = n_ext); .glob: the global row of each local id
    in [-n_front, n_ext) (index local + n_front); .own: this rank's global rows."""

    def __init__(self, mpg, A, row_starts, rank):
        r0, r1 = int(row_starts[rank]), int(row_starts[rank + 1])
        p0, p1 = int(A.rowptr[r0]), int(A.rowptr[r1])
        gcol = np.ascontiguousarray(A.col[p0:p1], np.int32)
        rp = np.ascontiguousarray(A.rowptr[r0:r1 + 1] - p0, np.int32)
        val = np.ascontiguousarray(A.val[p0:p1], np.float64)
        plan = mpg.HaloPlan(rank, len(row_starts) - 1, np.asarray(row_starts, np.int64),
                            mpg.Csr(r1 - r0, A.ncols, rp, gcol, val))
        self.n, self.n_ext, self.n_front = r1 - r0, plan.n_ext, plan.n_front
        lcol = plan.local_cols()
        plan.close()
        self.A = mpg.Csr(self.n, self.n_ext, rp, lcol, val)
        self.glob = np.full(self.n_front + self.n_ext, -1, np.int64)
        self.glob[lcol.astype(np.int64) + self.n_front] = gcol
        self.glob[self.n_front:self.n_front + self.n] = np.arange(r0, r1)
        assert np.all(self.glob >= 0), "a halo id no column uses"
        self.own = np.arange(r0, r1)

    def to_scipy(self):
        """n x (n_front + n_ext), the columns shifted by n_front."""
        import scipy.sparse as sp

        return sp.csr_matrix((self.A.val, self.A.col.astype(np.int64) + self.n_front, self.A.rowptr),
                             shape=(self.n, self.n_front + self.n_ext))


def front_pad(n_front):
    """MPG_FRONT_PAD of arnoldi.h: entries allocated in front of row 0 of a vector with a lower halo."""
    return (n_front + 63) // 64 * 64 + 64 if n_front > 0 else 0


def ld_of(n, itemsize):
    """mpg_arnoldi_create's leading dimension: columns padded to 256 B
    (asserted against the workspace's own in PhaseWorkspace)."""
    a = 256 // itemsize
    return (n + a - 1) // a * a


_P, _I = C.c_void_p, C.c_int
_DECLS = {  # what the package's own table leaves undeclared
    "reduce": [_P, _I], "cgs": [_P, _I, _I], "cgs_givens": [_P, _I, _I], "cgsr_wide_pass": [_P, _I, _I],
    "mgs": [_P, _I, _I], "mgs_partials": [_P, _I, _I], "givens": [_P, _I], "dots_sums": [_P, _I],
    "spmv_dots": [_P, _I, _I], "spmv_dots_supported": [_P, _I], "step_dots": [_P, _I, _I],
    "step_dots_supported": [_P, _I], "cgs_stream_at": [_P, _I], "prologue_finish": [_P], "slices_per_wave": [_P],
    "num_groups": [_P], "accum": [_P], "partials_count": [_P], "prologue_format": [_P],
    "sell_columns": [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "prec_fused": [_P, _I], "uniform_groups": [_P],
}


def _declare(lib):
    for name, args in _DECLS.items():
        fn = getattr(lib, "mpg_arnoldi_" + name)
        fn.argtypes, fn.restype = args, C.c_int


class DeviceCsr:
    """A's structure and its values of one type on the device (CSR row blocks)."""

    def __init__(self, hip, A, t):
        self.hip = hip
        self.rp, self.col = hip.buf(A.rowptr, np.int32), hip.buf(A.col, np.int32)
        self.csr = C.c_void_p()
        hip.call("mpg_csr_create", A.nrows, A.ncols, A.nnz, A.rowptr.ctypes.data, self.rp.p, self.col.p,
                 C.byref(self.csr))
        self.vals = hip.buf(A.val.astype(TYPES[t][0]))

    def close(self):
        self.hip.lib.mpg_csr_destroy(self.csr)
        for b in (self.rp, self.col, self.vals):
            b.free()


class PhaseWorkspace:
    """mpg_arnoldi_create on A. The defaults are those of the workspace the
    polynomial-preconditioner tests build (tests/test_neumann_gpu.py): m = 4,
    CGS, no preconditioner inside the launches, Jacobi's inverse diagonal in
    the descriptor, b = 1, x = 0, an fp64 residual, and 1/h = 1.

    storage: an object with .csr and .vals (A's values in T) to build on;
    else the workspace makes and owns one. MPG_CGS_PREFETCH and MPG_SELL_PAIR
    are read at create: set them (monkeypatch) first.

    Halo rows (n_ext > n, n_front > 0): A holds one rank's rows with local
    column ids in [-n_front, n_ext) and A.ncols = n_ext, as the row-partitioned
    engine passes them (host/fused_gmres.cpp); x has front_pad(n_front) + n_ext
    entries and the descriptor points at its row 0. The ext=True forms of
    put_w / get_w / put_x / get_x cover [-n_front, n_ext); the put forms also
    fill the pad in front of -n_front (`pad`).
    inner_val=MPG_F16: the Arnoldi values are mpg_csr_half_values' copy of A's
    fp64 values, scaled per row (row_exp=1) or not (0); the exponents go into
    the descriptor only when a row was scaled, as the engine does.
    prec_block: mpg_bjacobi_setup_*'s inverses of the diagonal blocks go into
    the descriptor as block_dinv (jacobi must be 0)."""

    def __init__(self, mpg, hip, A, t="f32", spmv_format=1, accum=0, *, m=4, orth=0, jacobi=0, basis=0, x=None,
                 b=None, storage=None, n_ext=None, n_front=0, inner_val=None, row_exp=1, prec_block=0):
        from mpgmres_amd._abi import ArnoldiDesc

        _declare(hip.lib)
        self.hip, self.lib, self.n, self.t, self.m = hip, hip.lib, A.nrows, t, m
        self.T, self.ct, vt = TYPES[t]
        self.own = storage is None
        self.S = DeviceCsr(hip, A, t) if storage is None else storage
        n = self.n
        self.val64 = hip.buf(A.val)
        self.diag = hip.buf(n, self.T)
        hip.call(f"mpg_jacobi_setup_{t}", self.S.csr, self.S.vals.p, self.diag.p)
        self.b = hip.buf(np.ones(n) if b is None else np.asarray(b, np.float64))
        self.n_ext, self.n_front = n if n_ext is None else n_ext, n_front
        self.front = front_pad(n_front)
        assert self.n_ext >= n and n_front >= 0 and A.ncols == self.n_ext, (n, self.n_ext, n_front, A.ncols)
        self.x = hip.buf(np.zeros(self.front + self.n_ext))
        self.xp = self.x.p.value + 8 * self.front  # row 0
        if x is not None:
            self.put_x(x, ext=len(x) != n)
        d = ArnoldiDesc()
        d.n, d.n_ext, d.n_front, d.m, d.orth = n, self.n_ext, n_front, m, ORTH.get(orth, orth)
        d.vec_type = d.prec_type = d.inner_val = vt
        d.outer_type = MPG_F64
        d.jacobi = jacobi
        d.A = self.S.csr.value
        d.val_outer = (self.val64 if t == "f32" else self.S.vals).p.value
        d.val_inner = self.S.vals.p.value
        d.diag = self.diag.p.value
        d.b, d.x = self.b.p.value, self.xp
        d.spmv_format = spmv_format
        self.half = self.rexp = self.dinv = None
        if inner_val == MPG_F16:
            self.half, self.rexp = hip.buf(A.nnz, np.uint16), hip.buf(n + 64, np.int8)
            stats = (C.c_int64 * 4)()
            self._check(self.lib.mpg_csr_half_values(hip.ctx, self.S.csr, self.val64.p, row_exp, self.half.p,
                                                     self.rexp.p if row_exp else None, stats), "mpg_csr_half_values")
            self.half_stats = list(stats)
            d.inner_val, d.val_inner = MPG_F16, self.half.p.value
            if row_exp and stats[0] > 0:  # rows all in range: the unscaled kernels (host/fused_gmres.cpp)
                d.inner_row_exp = self.rexp.p.value
        if prec_block:
            self.dinv = hip.buf(np.zeros(n * prec_block, self.T))
            bad = C.c_int32(-7)
            self._check(getattr(self.lib, f"mpg_bjacobi_setup_{t}")(hip.ctx, self.S.csr, self.S.vals.p, prec_block,
                                                                    self.dinv.p, C.byref(bad)), "mpg_bjacobi_setup")
            assert bad.value == -1, f"mpg_bjacobi_setup: diagonal block {bad.value} is singular"
            d.block_dinv, d.prec_block = self.dinv.p.value, prec_block
        self.arn = C.c_void_p()
        try:  # (a HIP runtime error ends the session in _check; a refused descriptor raises RuntimeError)
            self._check(self.lib.mpg_arnoldi_create(hip.ctx, C.byref(d), C.byref(self.arn)), "mpg_arnoldi_create")
        except RuntimeError:  # nothing of a refused descriptor stays behind
            self.close()
            raise
        hip.check(self.lib.mpg_arnoldi_set_accum(self.arn, accum), "set_accum")
        if basis:
            hip.check(self.lib.mpg_arnoldi_set_basis(self.arn, basis), "set_basis")
        self.basis = basis
        self.acc32 = self.lib.mpg_arnoldi_accum(self.arn) == 1
        f, win = C.c_int32(), C.c_int32()
        hip.check(self.lib.mpg_arnoldi_spmv_layout(self.arn, C.byref(f), None, None, None, C.byref(win)), "layout")
        self.format, self.window = f.value, win.value
        ld = C.c_int64()
        self._V = self.lib.mpg_arnoldi_basis_dev(self.arn, C.byref(ld))
        self.ld = ld.value
        self.VT = np.dtype(np.uint16) if basis == 1 else np.dtype(self.T)  # MPG_BASIS_F16: the stored fp16 bits
        assert self.ld == ld_of(n, self.VT.itemsize), (self.ld, n)
        self.put_inv(1)  # the Arnoldi SpMV then forms A w_prev itself

    def _check(self, st, what):
        """hip.check, except that a HIP runtime error (a fault: the device may be
        unusable) ends the whole session: nothing more is launched behind it."""
        if st == MPG_ERR_HIP:
            import pytest

            err = self.lib.mpg_ctx_last_error(self.hip.ctx)
            pytest.exit(f"{what}: HIP runtime error {err.decode() if err else ''}; session ended", returncode=3)
        self.hip.check(st, what)

    # ---- raw copies
    def _put(self, ptr, arr, dtype, offset=0):
        arr = np.ascontiguousarray(arr, dtype)
        assert ptr, "null device pointer"
        self._check(self.lib.mpg_memcpy_h2d(self.hip.ctx, C.c_void_p(ptr + offset * arr.itemsize), arr.ctypes.data,
                                               arr.nbytes), "h2d")

    def _get(self, ptr, count, dtype, offset=0):
        out = np.empty(count, dtype)
        assert ptr, "null device pointer"
        self._check(self.lib.mpg_memcpy_d2h(self.hip.ctx, out.ctypes.data,
                                               C.c_void_p(ptr + offset * out.itemsize), out.nbytes), "d2h")
        return out

    # ---- state
    def put_V(self, V):
        """Columns 0 .. V.shape[1] - 1, each ld entries (padding included)."""
        assert V.shape[0] == self.ld and V.shape[1] <= self.m + 1 and V.dtype == self.VT, (V.shape, V.dtype)
        self._put(self._V, np.asfortranarray(V).ravel(order="F"), self.VT)

    def get_V(self, j):
        return self._get(self._V, self.n, self.VT, j * self.ld)

    def _ext(self, v, pad):
        """[-front_pad, n_ext) from the n_front + n_ext entries of v, `pad` in front of -n_front."""
        assert len(v) == self.n_front + self.n_ext
        return np.concatenate([np.full(self.front - self.n_front, pad), np.asarray(v, np.float64)])

    def put_w(self, k, w, ext=False, pad=np.nan):
        """The input vector of step k (the other buffer is step k's output).
        ext: rows [-n_front, n_ext), and `pad` in the entries in front of them."""
        ptr = self.lib.mpg_arnoldi_wprev_dev(self.arn, k)
        if ext:
            return self._put(ptr, self._ext(w, pad), self.T, -self.front)
        assert len(w) == self.n
        self._put(ptr, w, self.T)

    def get_w(self, k, ext=False):
        ptr = self.lib.mpg_arnoldi_wprev_dev(self.arn, k)
        if ext:
            return self._get(ptr, self.n_front + self.n_ext, self.T, -self.n_front)
        return self._get(ptr, self.n, self.T)

    def put_H(self, H):
        assert H.shape == (self.m + 1, self.m)
        self._put(self.lib.mpg_arnoldi_hessenberg_dev(self.arn), np.asfortranarray(H).ravel(order="F"), self.T)

    def get_H(self):
        h = self._get(self.lib.mpg_arnoldi_hessenberg_dev(self.arn), (self.m + 1) * self.m, self.T)
        return h.reshape((self.m + 1, self.m), order="F")

    def put_rot(self, which, v):
        """which: 0 cs, 1 sn, 2 s; m + 1 values."""
        assert len(v) == self.m + 1
        self._put(self.lib.mpg_arnoldi_rotations_dev(self.arn, which), v, self.T)

    def get_rot(self, which):
        return self._get(self.lib.mpg_arnoldi_rotations_dev(self.arn, which), self.m + 1, self.T)

    def put_inv(self, v):
        self._put(self.lib.mpg_arnoldi_inv_dev(self.arn), np.array([v]), self.T)

    def get_inv(self):
        return self._get(self.lib.mpg_arnoldi_inv_dev(self.arn), 1, self.T)[0]

    def put_sums(self, v):
        assert len(v) <= self.m + 4
        self._put(self.lib.mpg_arnoldi_sums_dev(self.arn), v, np.float64)

    def get_sums(self, count):
        assert count <= self.m + 4
        return self._get(self.lib.mpg_arnoldi_sums_dev(self.arn), count, np.float64)

    def put_report(self, v):
        assert len(v) <= self.m + 4
        self._put(self.lib.mpg_arnoldi_report_dev(self.arn), v, np.float64)

    def get_report(self):
        return self._get(self.lib.mpg_arnoldi_report_dev(self.arn), self.lib.mpg_arnoldi_report_len(self.arn),
                         np.float64)

    def put_x(self, x, ext=False, pad=np.nan):
        if ext:
            return self._put(self.xp, self._ext(x, pad), np.float64, -self.front)
        assert len(x) == self.n
        self._put(self.xp, x, np.float64)

    def get_x(self, ext=False):
        if ext:
            return self._get(self.xp, self.n_front + self.n_ext, np.float64, -self.n_front)
        return self._get(self.xp, self.n, np.float64)

    def put_b(self, b):
        assert len(b) == self.n
        self._put(self.b.p.value, b, np.float64)

    def get_b(self):
        return self.b.get()

    # ---- launches
    def launch(self, name, *args):
        """mpg_arnoldi_<name>(workspace, *args), through hip.check."""
        self._check(getattr(self.lib, "mpg_arnoldi_" + name)(self.arn, *args), "mpg_arnoldi_" + name)

    def expect(self, query, args, value):
        """The table's expectation of a _supported / _at query: asserted, never skipped."""
        got = getattr(self.lib, "mpg_arnoldi_" + query)(self.arn, *args)
        assert got == value, (query, args, got, value)

    def launch_if(self, name, query, qargs, *args):
        """A form with a query: launched only after the query said MPG_OK."""
        self.expect(query, qargs, MPG_OK)
        self.launch(name, *args)

    def reduce(self, ncols):
        self.launch("reduce", ncols)
        return self.get_sums(ncols)

    def groups(self):
        return self.lib.mpg_arnoldi_num_groups(self.arn)

    def sell_form(self):
        form = C.c_int32()
        self.hip.check(self.lib.mpg_arnoldi_sell_columns(self.arn, C.byref(form), None, None), "sell_columns")
        return form.value

    def prec_fused(self, which):
        """mpg_arnoldi_prec_fused: 1 when the launches of `which` (0 the SpMV, 1 the prologue) apply block_dinv."""
        return self.lib.mpg_arnoldi_prec_fused(self.arn, which)

    def uniform_groups(self):
        """As the row-partitioned engine does once after create: the same partial count on every rank."""
        self._check(self.lib.mpg_arnoldi_uniform_groups(self.arn), "mpg_arnoldi_uniform_groups")

    def half_bits(self):
        """The device's fp16 copy of the values (CSR order)."""
        return self._get(self.half.p.value, self.half.n, np.uint16)

    def row_exp(self):
        """The device's per-row exponents of the fp16 copy."""
        return self._get(self.rexp.p.value, self.n, np.int8)

    def block_dinv(self):
        """The device's inverses of the diagonal blocks (prec_block values per row, row-major per block)."""
        return self._get(self.dinv.p.value, self.dinv.n, self.T)

    def sell_columns(self):
        """(form, CSR-summed slices) of mpg_arnoldi_sell_columns."""
        form, exc = C.c_int32(), C.c_int64()
        self._check(self.lib.mpg_arnoldi_sell_columns(self.arn, C.byref(form), C.byref(exc), None), "sell_columns")
        return form.value, exc.value

    def close(self):
        self.lib.mpg_arnoldi_destroy(self.arn)
        if self.own:
            self.S.close()
        for buf in (self.val64, self.diag, self.b, self.x, self.half, self.rexp, self.dinv):
            if buf is not None:
                buf.free()
