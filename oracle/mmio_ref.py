"""ORACLE — test infrastructure only. Never imported by the product.

The reference's Matrix Market reading, run with the reference's own parser:
mm_read_banner / mm_read_mtx_crd_size from /root/reference/mmio.c compiled
as-is into oracle/_ref/libmmio_ref.so (oracle/Makefile), and the entry loop
of LoadMatrix.hpp:62-80 through libc's fscanf with its exact format. The CSR
assembly that follows in LoadMatrix.hpp:82-146 (a diagonal slot per row,
symmetric mirroring, then a per-row bubble sort on the column) is restated
here in Python. tests/test_mmio_ref.py compares mpg_load_mtx with it.

Where the library is not built (no reference tree to compile from) the
parser's answers are replayed from tests/golden/mmio_ref_headers.json: for
each header the tests feed it, the bytes the reference's readers consumed,
their return codes, the type code and the sizes, recorded from the library
itself. Where it is built, every live answer is also held against its record,
so the two cannot drift apart; MPG_MMIO_RECORD=1 writes the missing records
(`MPG_MMIO_RECORD=1 python -m pytest tests/test_mmio_ref.py`).
"""
import ctypes as C
import json
import os
from pathlib import Path

import numpy as np

LIB = Path(__file__).resolve().parent / "_ref" / "libmmio_ref.so"
RECORDS = Path(__file__).resolve().parent.parent / "tests" / "golden" / "mmio_ref_headers.json"
# mmio.h:79-85
MM_PREMATURE_EOF, MM_NO_HEADER, MM_UNSUPPORTED_TYPE = 12, 14, 15

_libc = C.CDLL(None)
_libc.fopen.restype = C.c_void_p
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fclose.argtypes = [C.c_void_p]
_libc.ftell.restype = C.c_long
_libc.ftell.argtypes = [C.c_void_p]
_libc.fseek.argtypes = [C.c_void_p, C.c_long, C.c_int]


def available() -> bool:
    return LIB.exists()


def _lib():
    lib = C.CDLL(str(LIB))
    lib.mm_read_banner.argtypes = [C.c_void_p, C.c_char_p]
    lib.mm_read_mtx_crd_size.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 3
    lib.mm_read_mtx_array_size.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 2
    return lib


def _live_header(f, vector: bool) -> dict:
    """mm_read_banner, then the size reader its caller uses: LoadMatrix
    mm_read_mtx_crd_size; LoadVector mm_read_mtx_array_size for an array
    file, mm_read_mtx_crd_size otherwise. The file is left where they stop."""
    lib = _lib()
    h = {"reader": None, "banner_err": 0, "code": "", "size_err": None, "M": 0, "N": 0, "nnz": 0}
    code = C.create_string_buffer(4)
    h["banner_err"] = lib.mm_read_banner(f, code)
    if not h["banner_err"]:
        h["code"] = code.raw.decode("latin-1")
        M, N, nnz = C.c_int(), C.c_int(), C.c_int()
        h["reader"] = "array" if vector and h["code"][1] == "A" else "crd"
        h["size_err"] = (lib.mm_read_mtx_array_size(f, C.byref(M), C.byref(N)) if h["reader"] == "array"
                         else lib.mm_read_mtx_crd_size(f, C.byref(M), C.byref(N), C.byref(nnz)))
        if not h["size_err"]:
            h.update(M=M.value, N=N.value, nnz=nnz.value)
    return h


def _header(f, path: str, vector: bool) -> dict:
    """The reference readers' answer for this file's header (live, and held
    against its record; or the record alone), as _live_header's dict. A
    record fits a file that begins with the bytes the readers consumed (and
    ends there, if the recorded one did) under the same size reader."""
    data = Path(path).read_bytes()
    records = json.loads(RECORDS.read_text()) if RECORDS.exists() else []
    fits = [r for r in records
            if data.startswith(r["consumed"].encode("latin-1")) and r["at_eof"] == (len(data) == len(r["consumed"]))
            and (r["reader"] is None or (r["reader"] == "array") == (vector and r["code"][1] == "A"))]
    rec = max(fits, key=lambda r: len(r["consumed"]), default=None)
    if not available():
        assert rec is not None, f"no recorded reference header fits {path}: record it where oracle/_ref is built"
        _libc.fseek(f, len(rec["consumed"]), 0)
        return rec
    h = _live_header(f, vector)
    at = _libc.ftell(f)
    h.update(consumed=data[:at].decode("latin-1"), at_eof=at >= len(data))
    if rec is None and os.environ.get("MPG_MMIO_RECORD") == "1":
        RECORDS.write_text(json.dumps(records + [h], indent=1) + "\n")
        rec = h
    assert rec == h, f"the recorded reference header for {path} is {rec}, the library says {h}"
    return h


_BANNER_ERRORS = {MM_PREMATURE_EOF: "Missing values in banner", MM_NO_HEADER: "Banner is missing",
                  MM_UNSUPPORTED_TYPE: "Unrecognized description"}


def load_matrix(path: str):
    """LoadMatrix<double>(file) (LoadMatrix.hpp:17-154): returns (M, N,
    rowptr, col, val) or raises ValueError with the reference's message."""
    f = _libc.fopen(str(path).encode(), b"r")
    if not f:
        raise ValueError("Could not access file")
    try:
        h = _header(f, path, vector=False)
        if h["banner_err"]:
            raise ValueError(_BANNER_ERRORS.get(h["banner_err"], "Malformed banner with unknown error code"))
        if h["size_err"] != 0:
            raise ValueError("Malformed matrix size information")
        t = h["code"]
        # mm_is_coordinate && (real || integer) && (general || symmetric)
        if not (t[1] == "C" and t[2] in "RI" and t[3] in "GS"):
            raise ValueError("Unsupported matrix type")
        symmetric = t[3] == "S"
        M, N, nnz = h["M"], h["N"], h["nnz"]
        I, J, V = np.empty(nnz, np.int64), np.empty(nnz, np.int64), np.empty(nnz)
        ii, jj, vv = C.c_int(), C.c_int(), C.c_double()
        for k in range(nnz):  # LoadMatrix.hpp:67-70, fscanf(in, "%d %d %lg\n", ...)
            _libc.fscanf(C.c_void_p(f), b"%d %d %lg\n", C.byref(ii), C.byref(jj), C.byref(vv))
            I[k], J[k], V[k] = ii.value - 1, jj.value - 1, vv.value
    finally:
        _libc.fclose(f)
    return (M, N) + assemble(N, I, J, V, symmetric)


def assemble(N, I, J, V, symmetric):
    """LoadMatrix.hpp:61-146: every row gets a diagonal slot first (value 0
    unless the file sets it; a repeated diagonal keeps the last), off-diagonal
    entries (and their mirrors) follow in file order, then each row is bubble
    sorted on the column (stable: equal columns keep file order)."""
    off = I != J
    counts = np.ones(N, np.int64)
    np.add.at(counts, I[off], 1)
    if symmetric:
        np.add.at(counts, J[off], 1)
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum(counts)
    col = np.full(rowptr[-1], -1, np.int64)
    val = np.zeros(rowptr[-1])
    fill = np.ones(N, np.int64)
    col[rowptr[:-1]] = np.arange(N)
    for k in range(len(I)):
        r, c, v = int(I[k]), int(J[k]), V[k]
        if r == c:
            val[rowptr[r]] = v
            continue
        col[rowptr[r] + fill[r]], val[rowptr[r] + fill[r]] = c, v
        fill[r] += 1
        if symmetric:
            col[rowptr[c] + fill[c]], val[rowptr[c] + fill[c]] = r, v
            fill[c] += 1
    for r in range(N):  # the bubble sort is stable: a stable argsort gives the same order
        a, b = rowptr[r], rowptr[r + 1]
        order = np.argsort(col[a:b], kind="stable")
        col[a:b], val[a:b] = col[a:b][order], val[a:b][order]
    return rowptr, col, val


def load_vector(path: str, col: int = 0) -> np.ndarray:
    """LoadVector<double>(file, col) (LoadMatrix.hpp:156-233) with the
    reference's mmio.c banner/size readers and its fscanf formats."""
    f = _libc.fopen(str(path).encode(), b"r")
    if not f:
        raise ValueError("Could not access file")
    try:
        h = _header(f, path, vector=True)
        if h["banner_err"]:
            raise ValueError(_BANNER_ERRORS.get(h["banner_err"], "Malformed banner with unknown error code"))
        if h["size_err"]:
            raise ValueError("Malformed matrix size information")
        if col >= h["N"]:
            raise ValueError(f"Column {col} is too large for the {h['N']} vectors")
        out = np.zeros(h["M"])
        d = C.c_double()
        if h["reader"] == "array":  # LoadMatrix.hpp:197-209
            for _ in range(col * h["M"]):
                _libc.fscanf(C.c_void_p(f), b"%lf\n", C.byref(d))
            for j in range(h["M"]):
                _libc.fscanf(C.c_void_p(f), b"%lf\n", C.byref(d))
                out[j] = d.value
        else:  # LoadMatrix.hpp:210-222
            ii, jj = C.c_int(), C.c_int()
            for _ in range(h["nnz"]):
                _libc.fscanf(C.c_void_p(f), b"%d %d %lg\n", C.byref(ii), C.byref(jj), C.byref(d))
                if jj.value - 1 == col:
                    out[ii.value - 1] = d.value
    finally:
        _libc.fclose(f)
    return out
