"""The life cycle the streaming row analyses share: a device workspace sized and cleared through the C ABI, accumulate() calls that
take the sampler's post-burn-in rows [n][Q][stride][chains] in order, a segment at a time, and a result once every row is in.

RowAccumulator owns the device check, the workspace, the row check, the count of rows seen and free(); a subclass keeps its
constructor's arguments, the ABI call or calls of its analysis (_accumulate) and the shape of its result.

torch is imported where it is first needed, not with this module: pyhillfit_amd.sensitivity is imported by the command line to check
its arguments before torch is loaded."""
import ctypes as C

from . import _lib


def workspace_bytes(symbol, *shape):
    """the size the ABI's `symbol` (a phf_*_workspace_bytes) gives for `shape`; raises ValueError with its reason on an invalid shape"""
    lib = _lib.load()
    n = getattr(lib, symbol)(*(int(v) for v in shape))
    if n == 0:
        raise ValueError(lib.phf_last_error().decode())
    return int(n)


def check_tensor(rows, device):
    import torch
    if rows.dtype != torch.float64 or not rows.is_contiguous() or rows.device != device:
        raise ValueError("rows must be a contiguous float64 tensor on %s" % device)


def check_rows(rows, num_problems, chains, min_cols, device):
    """rows must be a contiguous float64 tensor [n][num_problems][>= min_cols][chains] on `device` (any tensors: needs no GPU)"""
    if rows.dim() != 4 or rows.shape[1] != num_problems or rows.shape[3] != chains or rows.shape[2] < min_cols:
        raise ValueError("rows must be [n][%d][>= %d][%d], got %s" % (num_problems, min_cols, chains, tuple(rows.shape)))
    check_tensor(rows, device)


class RowAccumulator(object):
    """Base of the streaming analyses.  A subclass sets Q, C and min_cols (the columns of a row it reads), N where the run has a
    known total of rows, lists its device tensors in `tensors` and implements _accumulate(rows, n)."""

    N = None                 # total post-burn-in rows; None: the analysis takes what comes (it thins the rows by `every`)
    tensors = ("ws",)        # what free() drops

    def __init__(self, device):
        import torch
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("%s runs on a GPU device, not %s" % (type(self).__name__, self.device))
        self.rows_seen = 0

    def _init_workspace(self, nbytes, init, *shape):
        """allocate nbytes and hand them to the ABI's `init` (a phf_*_init): shape..., workspace, bytes, stream"""
        import torch
        from .sampler import _ptr, _stream_ptr
        self.nbytes = nbytes
        self.ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device)
        _lib.check(getattr(self.lib, init)(*shape, _ptr(self.ws), C.c_size_t(nbytes), _stream_ptr(self.device)), init)

    def _check_rows(self, rows):
        check_rows(rows, self.Q, self.C, self.min_cols, self.device)

    def accumulate(self, rows):
        """rows: contiguous float64 device tensor [n][num_problems][stride >= columns read][chains], the next n post-burn-in rows"""
        self._check_rows(rows)
        n = rows.shape[0]
        if self.N is not None and self.rows_seen + n > self.N:
            raise ValueError("%d rows would exceed total_rows = %d" % (self.rows_seen + n, self.N))
        if n == 0:
            return None
        out = self._accumulate(rows, n)
        self.rows_seen += n
        return out

    def _check_complete(self):
        if self.rows_seen != self.N:
            raise ValueError("only %d of %d rows accumulated" % (self.rows_seen, self.N))

    def free(self):
        for name in self.tensors:
            setattr(self, name, None)
