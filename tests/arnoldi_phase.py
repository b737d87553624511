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

MPG_F64, MPG_F32 = 0, 1
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
    are read at create: set them (monkeypatch) first."""

    def __init__(self, mpg, hip, A, t="f32", spmv_format=1, accum=0, *, m=4, orth=0, jacobi=0, basis=0, x=None,
                 b=None, storage=None):
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
        self.x = hip.buf(np.zeros(n) if x is None else np.asarray(x, np.float64))
        d = ArnoldiDesc()
        d.n, d.n_ext, d.m, d.orth = n, n, m, ORTH.get(orth, orth)
        d.vec_type = d.prec_type = d.inner_val = vt
        d.outer_type = MPG_F64
        d.jacobi = jacobi
        d.A = self.S.csr.value
        d.val_outer = (self.val64 if t == "f32" else self.S.vals).p.value
        d.val_inner = self.S.vals.p.value
        d.diag = self.diag.p.value
        d.b, d.x = self.b.p.value, self.x.p.value
        d.spmv_format = spmv_format
        self.arn = C.c_void_p()
        hip.call("mpg_arnoldi_create", C.byref(d), C.byref(self.arn))
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

    def put_w(self, k, w):
        """The input vector of step k (the other buffer is step k's output)."""
        assert len(w) == self.n
        self._put(self.lib.mpg_arnoldi_wprev_dev(self.arn, k), w, self.T)

    def get_w(self, k):
        return self._get(self.lib.mpg_arnoldi_wprev_dev(self.arn, k), self.n, self.T)

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

    def put_x(self, x):
        assert len(x) == self.n
        self._put(self.x.p.value, x, np.float64)

    def get_x(self):
        return self.x.get()

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

    def close(self):
        self.lib.mpg_arnoldi_destroy(self.arn)
        if self.own:
            self.S.close()
        for buf in (self.val64, self.diag, self.b, self.x):
            buf.free()
