"""
Device engine: thin Python wrappers around libshg.  Arrays live on the GPU as torch tensors (fp64,
contiguous); every routine hands raw device pointers and the current HIP stream to the C ABI.

Nothing in here computes on the CPU: without the library or without a GPU the calls raise.
"""

import collections
import ctypes
import hashlib

import numpy as np

from . import _lib


def _torch():
    import torch
    return torch


def require_gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError('grates_amd: no GPU visible -- the hot path runs on MI355X only (there is no CPU fallback)')
    _lib.load()
    return torch


def device(index=None):
    torch = require_gpu()
    return torch.device('cuda', torch.cuda.current_device() if index is None else index)


def to_device(x, dev=None):
    """fp64 contiguous device tensor from ndarray / tensor / scalar sequence."""
    torch = require_gpu()
    dev = device() if dev is None else dev
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(dev)


def to_host(t):
    return t.detach().cpu().numpy()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _host_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class Plan:
    """
    Device tables for one (max_degree, parallels, kn table, meridians) configuration
    (shg_plan_create).  `colat` [nlat] geocentric colatitudes, `kn` [nlat, N+1], `meridians` [nlon].
    """

    def __init__(self, max_degree, colat, kn, meridians, device_index=None):
        torch = require_gpu()
        self.device = device(device_index)
        self.max_degree = int(max_degree)
        colat = np.ascontiguousarray(colat, dtype=np.float64)
        kn = np.ascontiguousarray(kn, dtype=np.float64)
        meridians = np.ascontiguousarray(meridians, dtype=np.float64)
        if kn.shape != (colat.size, self.max_degree + 1):
            raise ValueError('kn must have shape (nlat, max_degree + 1), got {0}'.format(kn.shape))
        self.nlat, self.nlon = colat.size, meridians.size
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.call('shg_plan_create', ctypes.byref(self._handle), self.max_degree, self.nlat, _host_ptr(colat),
                      _host_ptr(kn), self.nlon, _host_ptr(meridians), self.device.index)

    def __del__(self):
        handle = getattr(self, '_handle', None)
        if handle is not None and handle.value:
            try:
                _lib.load().shg_plan_destroy(handle)
            except Exception:
                pass
            self._handle = None             # (module globals may already be gone at interpreter shutdown)

    def info(self):
        arr = (ctypes.c_int64 * 8)()
        _lib.call('shg_plan_info', self._handle, arr)
        nblocks, enabled = ctypes.c_int(0), ctypes.c_int(0)
        _lib.call('shg_plan_order_cutoffs', self._handle, None, 0, ctypes.byref(nblocks), ctypes.byref(enabled))
        levels = (ctypes.c_int * max(nblocks.value, 1))()
        _lib.call('shg_plan_order_cutoffs', self._handle, levels, nblocks.value, ctypes.byref(nblocks), ctypes.byref(enabled))
        return {'max_degree': arr[0], 'nlat': arr[1], 'nlon': arr[2], 'fourfold_symmetry': bool(arr[3] & 1), 'north_south_symmetry': bool(arr[3] & 2),
                'rotation_symmetry': bool(arr[3] & 4), 'half_tile_fold': bool(arr[3] & 8), 'epochs_per_pass': arr[4], 'k_slots': arr[5], 'fused': bool(arr[6]), 'path': int(arr[7]) & 0xff, 'rotations': int(arr[7]) >> 8,
                'order_pruning': bool(enabled.value), 'order_cutoffs': [int(levels[i]) for i in range(nblocks.value)]}

    def set_path(self, path):
        """'auto', 'staged' (three kernels, any grid), 'fused' (single kernel on 4-fold symmetric meridians), 'fused32' (32-row
        panels) or 'rot' (rotation-folded kernel on equi-angular meridians with nlon % 96 == 0 or nlon % 48 == 0).  The fused
        kernels use the north-south symmetry of the parallels when the grid has it (their plain variants otherwise)."""
        _lib.call('shg_plan_set_path', self._handle, {'auto': 0, 'staged': 1, 'fused': 2, 'fused32': 5, 'rot': 6}[path])

    def set_stage_limit(self, limit):
        """Rotation-folded kernel only: at most `limit` workgroups in their Legendre stage at once (< 0: sixteenths of the CUs, 0 = off),
        kept per XCD by ticket queues.  A plan on which this was never called limits grids of more than one workgroup per CU to a
        share of the CUs that follows its shape (4/16 on the d/o 96 -> 0.25 degree headline)."""
        _lib.call('shg_plan_set_stage_limit', self._handle, int(limit))

    def set_order_pruning(self, enable):
        """Rotation-folded kernel only: latitude blocks next to a pole skip the orders that cannot reach them (on by default; off
        for comparisons).  `info()['order_cutoffs']` lists the largest order every block keeps."""
        _lib.call('shg_plan_set_order_pruning', self._handle, 1 if enable else 0)

    def set_half_tile_fold(self, enable):
        """Rotation-folded kernel only, where the fundamental domain has 8 mod 16 columns: the last column tile runs on 16 real columns
        and stores its ascending images only (on by default; off for comparisons: all 2 R images, the 8 columns beyond the domain
        dropped).  `info()['half_tile_fold']` tells whether the kernel folds that tile."""
        _lib.call('shg_plan_set_half_tile_fold', self._handle, 1 if enable else 0)

    def set_rotations(self, R):
        """Rotation count of the rotation-folded kernel: 0 (the plan's own choice), 3, 6, 9 or 10; the meridians must be invariant
        under R rotations with nlon / R a multiple of 16 (`info()['rotations']` tells the count in use)."""
        _lib.call('shg_plan_set_rotations', self._handle, int(R))

    def set_chunk(self, epochs_per_pass):
        _lib.call('shg_plan_set_chunk', self._handle, int(epochs_per_pass))

    PROFILE_KINDS = ('pack_coefficients', 'legendre_stage', 'lon_stage', 'covprop', 'analysis_lon', 'analysis_solve', 'k6', 'k7')

    def profile(self, enable=True, kinds=None):
        """Record HIP events around every kernel this plan launches (on the launching stream), or around the kernels of the named
        `kinds` only (PROFILE_KINDS; an event pair costs the stream ~5 us)."""
        if enable and kinds:
            mask = 0
            for name in kinds:
                mask |= 1 << (self.PROFILE_KINDS.index(name) + 1)
            _lib.call('shg_plan_profile', self._handle, mask)
        else:
            _lib.call('shg_plan_profile', self._handle, 1 if enable else 0)

    def profile_read(self):
        """{kernel: (total_ms, launches)} since the last read; synchronises the recorded events."""
        ms = (ctypes.c_double * 8)()
        n = (ctypes.c_int64 * 8)()
        _lib.call('shg_plan_profile_read', self._handle, ms, n)
        return {name: (ms[k], n[k]) for k, name in enumerate(self.PROFILE_KINDS) if n[k] > 0}

    def synthesis(self, anm, out=None):
        """anm [B, N+1, N+1] (or [N+1, N+1]), or an OrderMajorSeries of at least the plan's degree -> grid [B, nlat, nlon] (device tensor)."""
        torch = _torch()
        if isinstance(anm, OrderMajorSeries):
            B = anm.epochs
            if anm.max_degree < self.max_degree:
                raise ValueError('the series holds degrees up to {0}, the plan needs {1}'.format(anm.max_degree, self.max_degree))
            if out is None:
                out = torch.empty((B, self.nlat, self.nlon), dtype=torch.float64, device=self.device)
            elif tuple(out.shape) != (B, self.nlat, self.nlon) or out.dtype != torch.float64 or not out.is_contiguous():
                raise ValueError('out must be a contiguous fp64 tensor of shape {0}'.format((B, self.nlat, self.nlon)))
            Plan._written(out)
            with torch.cuda.device(self.device):
                try:
                    _lib.call('shg_synthesis_om', self._handle, _ptr(anm.data), anm.max_degree, B, anm.padded_epochs, _ptr(out), _stream())
                except _lib.ShgError:            # a plan whose kernel reads the reference arrays only: through them
                    batch = anm.to_batch()
                    n1 = self.max_degree + 1
                    _lib.call('shg_synthesis', self._handle, _ptr(batch[:, :n1, :n1].contiguous()), B, _ptr(out), _stream())
            return out
        x = to_device(anm, self.device)
        single = x.dim() == 2
        if single:
            x = x.unsqueeze(0)
        n1 = self.max_degree + 1
        if x.dim() != 3 or x.shape[1] != n1 or x.shape[2] != n1:
            raise ValueError('coefficient batch must have shape (B, {0}, {0}), got {1}'.format(n1, tuple(x.shape)))
        B = x.shape[0]
        if out is None:
            out = torch.empty((B, self.nlat, self.nlon), dtype=torch.float64, device=self.device)
        elif tuple(out.shape) != (B, self.nlat, self.nlon) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError('out must be a contiguous fp64 tensor of shape {0}'.format((B, self.nlat, self.nlon)))
        Plan._written(out)
        with torch.cuda.device(self.device):
            _lib.call('shg_synthesis', self._handle, _ptr(x), B, _ptr(out), _stream())
        return out[0] if single else out

    def covariance_propagation(self, cov, min_degree, lat0=0, lat1=None, symmetric=False, method='direct', out=None):
        """cov [P, P] degree-wise -> sigma [(lat1-lat0)*nlon] for the band of parallels [lat0, lat1), written to `out` when given.

        symmetric: False (default) multiplies with the full matrix like the reference; True reads only the upper triangle
        of a symmetric matrix (half the MFMA work; the other triangle may hold anything, NaN included); None checks the matrix
        on the device and takes the shortcut when it is exactly symmetric (the result then differs from the general path by
        summation order only; a NaN or an infinity on one side of the diagonal counts as not symmetric).
        method: 'direct' forms A Sigma like the reference (2 M P^2 flops on the MFMA units); 'separable' uses the
        factorisation of the synthesis matrix into a latitude and a longitude part (about nlon times fewer flops,
        P^2 + 32 P nlat doubles of workspace), same result up to summation order."""
        torch = _torch()
        lat1 = self.nlat if lat1 is None else lat1
        c = to_device(cov, self.device)
        P = (self.max_degree + 1) ** 2 - min_degree ** 2
        if c.dim() != 2 or c.shape[0] != P or c.shape[1] != P:
            raise ValueError('covariance matrix must have shape ({0}, {0}), got {1}'.format(P, tuple(c.shape)))
        if out is None:
            out = torch.empty(((lat1 - lat0) * self.nlon,), dtype=torch.float64, device=self.device)
        elif tuple(out.shape) != ((lat1 - lat0) * self.nlon,) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != c.device:
            raise ValueError('out must be a contiguous fp64 tensor of shape {0} on the plan\'s device'.format(((lat1 - lat0) * self.nlon,)))
        if method not in ('direct', 'separable'):
            raise ValueError("method must be 'direct' or 'separable'")
        with torch.cuda.device(self.device):
            if symmetric is None:
                defect = torch.zeros(1, dtype=torch.float64, device=self.device)
                _lib.call('shg_symmetry_defect', _ptr(c), P, P, _ptr(defect), _stream())
                symmetric = float(defect.item()) == 0.0
            if method == 'separable':
                _lib.call('shg_covprop_diag_separable_symmetric' if symmetric else 'shg_covprop_diag_separable', self._handle, _ptr(c),
                          int(min_degree), int(lat0), int(lat1), _ptr(out), _stream())
                return out
            _lib.call('shg_covprop_diag_symmetric' if symmetric else 'shg_covprop_diag', self._handle, _ptr(c), int(min_degree), int(lat0), int(lat1),
                      _ptr(out), _stream())
        return out

    _trusting = None          # weak set of the plans that hold a weight token (class attribute, created on first use)

    @classmethod
    def _written(cls, tensor):
        """A library call is about to write into `tensor` through its raw pointer (torch's version counter does not see that): plans
        that trust weights living in the same storage forget their token and validate the weights again on their next analysis."""
        if not cls._trusting:
            return
        try:
            storage = tensor.untyped_storage().data_ptr()
        except Exception:
            return
        for plan in list(cls._trusting):
            w = plan._analysis_weights
            if w is not None and w.untyped_storage().data_ptr() == storage:
                plan._analysis_token = None

    def analysis(self, grid, area, min_degree, trusted_weights=None):
        """grid [B, nlat, nlon], area [nlat, nlon] -> anm [B, N+1, N+1].

        The library validates `area` against the weights its cached operators were built for on every call (a device compare and
        one host synchronisation).  A device tensor that is the very tensor of the previous call (same storage, same torch
        version counter: not written to since) need not be compared again -- the call then passes area = NULL ("the weights of
        the previous call", include/shg.h) and nothing waits for the device.  Writes through `.data` or through raw pointers outside
        this module are invisible to the version counter: `trusted_weights=False` always validates, `True` skips the validation
        whatever the tensor's history (the caller vouches for it); this module's own raw-pointer writes (`gemm(out=)`, `axpby`,
        `Plan.synthesis(out=)`) into the storage of trusted weights withdraw the trust."""
        torch = _torch()
        g = to_device(grid, self.device)
        single = g.dim() == 2
        if single:
            g = g.unsqueeze(0)
        n1 = self.max_degree + 1
        out = torch.empty((g.shape[0], n1, n1), dtype=torch.float64, device=self.device)    # zeroed by the library
        token = None
        if torch.is_tensor(area) and area.is_cuda and area.dtype == torch.float64 and area.is_contiguous():
            token = (area.data_ptr(), area._version, tuple(area.shape), int(min_degree))
        with torch.cuda.device(self.device):
            trusted = token is not None and (token == self._analysis_token if trusted_weights is None else
                                             (bool(trusted_weights) and self._analysis_token is not None and token[2:] == self._analysis_token[2:]))
            if g.shape[0] > 0 and trusted and trusted_weights is not False:
                _lib.call('shg_analysis', self._handle, _ptr(g), None, int(min_degree), g.shape[0], _ptr(out), _stream())
            else:
                a = to_device(area, self.device).reshape(self.nlat, self.nlon)
                self._analysis_token = None
                _lib.call('shg_analysis', self._handle, _ptr(g), _ptr(a), int(min_degree), g.shape[0], _ptr(out), _stream())
                if g.shape[0] > 0:       # (the tensor is kept alive: its address cannot be handed to another one meanwhile)
                    self._analysis_token, self._analysis_weights = token, (area if token is not None else None)
                    if token is not None:
                        import weakref
                        if Plan._trusting is None:
                            Plan._trusting = weakref.WeakSet()
                        Plan._trusting.add(self)
        return out[0] if single else out

    _analysis_token = None
    _analysis_weights = None

    def analysis_info(self):
        """{'parity_split': True | False | None (no operators yet), 'parity_defect': float} of the cached analysis operators (include/shg.h)"""
        info = (ctypes.c_double * 2)()
        _lib.call('shg_analysis_info', self._handle, ctypes.addressof(info))
        return {'parity_split': None if info[0] < 0 else bool(info[0]), 'parity_defect': float(info[1])}

    def analysis_matrix(self, area, min_degree):
        """Dense analysis operator F [P, nlat * nlon] (device tensor) for the area weights `area`: F @ values = analysis(values)."""
        torch = _torch()
        self._analysis_token = None                    # the call may rebuild the cached operators for other weights
        a = to_device(area, self.device).reshape(self.nlat, self.nlon)
        P = (self.max_degree + 1) ** 2 - min_degree ** 2
        out = torch.empty((P, self.nlat * self.nlon), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call('shg_analysis_matrix', self._handle, _ptr(a), int(min_degree), _ptr(out), _stream())
        return out


def release_scratch():
    """Give the per-stream scratch buffers the library keeps between calls (shg_analysis, split-K block products) back to
    the driver; waits for the device."""
    require_gpu()
    _lib.call('shg_scratch_release')


_plan_cache = {}
_PLAN_CACHE_LIMIT = 8


def cached_plan(max_degree, colat, kn, meridians):
    """Plans are cached by content so that repeated to_grid calls reuse the device tables."""
    torch = require_gpu()
    h = hashlib.blake2b(digest_size=16)
    for a in (np.int64(max_degree), np.int64(torch.cuda.current_device()), colat, kn, meridians):
        h.update(np.ascontiguousarray(a).tobytes())
    key = h.hexdigest()
    plan = _plan_cache.pop(key, None)
    if plan is None:
        if len(_plan_cache) >= _PLAN_CACHE_LIMIT:
            _plan_cache.pop(next(iter(_plan_cache)))           # least recently used: a hit moves its plan to the end
        plan = Plan(max_degree, colat, kn, meridians)
    _plan_cache[key] = plan
    return plan


_grid_plan_cache = {}


def plan_by_grid(scalars, axes, build):
    """The plan of a regular grid found by what defines it -- kernel name, degree, constants (`scalars`, hashable) and the two axes
    (`axes`: parallels, meridians; hashed: 17 KB on the 0.25 degree grid) -- without building the kernel table first; `build()` makes
    the plan on a miss.  Least recently used of _PLAN_CACHE_LIMIT entries goes first."""
    torch = require_gpu()
    h = hashlib.blake2b(digest_size=16)
    h.update(repr((scalars, torch.cuda.current_device())).encode())
    for a in axes:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    key = h.hexdigest()
    plan = _grid_plan_cache.pop(key, None)
    if plan is None:
        if len(_grid_plan_cache) >= _PLAN_CACHE_LIMIT:
            _grid_plan_cache.pop(next(iter(_grid_plan_cache)))
        plan = build()
    _grid_plan_cache[key] = plan
    return plan


_table_cache = {}


def cached_point_tables(max_degree, latitude, longitude, tag, build):
    """Device copies of the per-point tables (colatitude, longitude, degree factors) of a point list, cached by content like
    the plans: `build()` -> (colat, lon, kn) host arrays is only called for a new (points, kernel / constants tag, degree)."""
    torch = require_gpu()
    h = hashlib.blake2b(digest_size=16)
    h.update(repr((int(max_degree), int(torch.cuda.current_device()), tag)).encode())
    for a in (latitude, longitude):
        h.update(np.ascontiguousarray(a).tobytes())
    key = h.hexdigest()
    entry = _table_cache.get(key)
    if entry is None:
        if len(_table_cache) >= _PLAN_CACHE_LIMIT:
            _table_cache.pop(next(iter(_table_cache)))
        entry = tuple(to_device(a) for a in build())
        _table_cache[key] = entry
    return entry


def clear_plan_cache():
    _plan_cache.clear()
    _table_cache.clear()


# ---------------------------------------------------------------------------------------------------
# table functions / index maps
# ---------------------------------------------------------------------------------------------------

def legendre_functions(max_degree, colat):
    torch = require_gpu()
    th = to_device(np.atleast_1d(colat))
    out = torch.empty((th.numel(), max_degree + 1, max_degree + 1), dtype=torch.float64, device=th.device)
    _lib.call('shg_legendre', int(max_degree), _ptr(th), th.numel(), _ptr(out), _stream())
    return out


def legendre_functions_per_order(max_degree, order, colat):
    torch = require_gpu()
    th = to_device(np.atleast_1d(colat))
    out = torch.empty((th.numel(), max_degree + 1 - order), dtype=torch.float64, device=th.device)
    _lib.call('shg_legendre_order', int(max_degree), int(order), _ptr(th), th.numel(), _ptr(out), _stream())
    return out


def trigonometric_functions(max_degree, lon):
    torch = require_gpu()
    lam = to_device(np.atleast_1d(lon))
    out = torch.empty((lam.numel(), max_degree + 1, max_degree + 1), dtype=torch.float64, device=lam.device)
    _lib.call('shg_trigonometric', int(max_degree), _ptr(lam), lam.numel(), _ptr(out), _stream())
    return out


def synthesis_matrix_order(max_degree, order, min_degree, colat, lon, kn, pointwise):
    """Operator block of one order (device tensors): (cosine block, sine block or None for order 0), rows parallel-major for a
    regular grid (pointwise=False: colat / kn per parallel, lon = meridians) or one row per point (pointwise=True)."""
    torch = require_gpu()
    th, lam, k = to_device(np.atleast_1d(colat)), to_device(np.atleast_1d(lon)), to_device(kn)
    nlat, nlon = th.numel(), lam.numel()
    if k.shape != (nlat, max_degree + 1) or (pointwise and nlon != nlat):
        raise ValueError('synthesis_matrix_order: colat [k], kn [k, max_degree + 1] and, for point lists, lon [k] expected')
    count = max_degree + 1 - max(order, min_degree)
    rows = nlat if pointwise else nlat * nlon
    out_c = torch.empty((rows, max(count, 0)), dtype=torch.float64, device=th.device)
    out_s = torch.empty_like(out_c) if order > 0 else None
    _lib.call('shg_synthesis_matrix_order', int(max_degree), int(order), int(min_degree), _ptr(th), nlat, _ptr(lam), nlon, _ptr(k),
              1 if pointwise else 0, _ptr(out_c), _ptr(out_s) if out_s is not None else None, _stream())
    return out_c, out_s


def synthesis_matrix(max_degree, min_degree, colat, lon, kn):
    """Dense synthesis operator A [npts, P] (device tensor) of the points (colat, lon) with degree factors kn [npts, N+1]."""
    torch = require_gpu()
    th, lam, k = to_device(np.atleast_1d(colat)), to_device(np.atleast_1d(lon)), to_device(kn)
    npts = th.numel()
    if k.shape != (npts, max_degree + 1) or lam.numel() != npts:
        raise ValueError('synthesis_matrix: colat, lon [npts] and kn [npts, max_degree + 1] expected')
    P = (max_degree + 1) ** 2 - min_degree ** 2
    out = torch.empty((npts, P), dtype=torch.float64, device=th.device)
    _lib.call('shg_synthesis_matrix', int(max_degree), int(min_degree), _ptr(th), _ptr(lam), _ptr(k), npts, _ptr(out), _stream())
    return out


# ---------------------------------------------------------------------------------------------------
# sparse block Cholesky (csrc/blockchol.hip): block tables are [nb, nb] uint64 arrays of device addresses (0 = no block)
# ---------------------------------------------------------------------------------------------------

def _table(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


class BlockTable:
    """Stored upper blocks of a block matrix in compressed row form for the shg_block_* calls (include/shg.h):
    `blocks` maps (i, j), j >= i, to a device tensor [rows_i, cols_j]."""

    def __init__(self, bounds, blocks):
        self.bounds = np.ascontiguousarray(bounds, dtype=np.int32)
        nb = self.bounds.size - 1
        keys = sorted(k for k in blocks if k[1] >= k[0])
        for k in keys:                   # csrc/blockchol.hip reads every block as dense row-major with ld = columns
            if not blocks[k].is_contiguous():
                raise ValueError('block {0} is not a contiguous row-major tensor (strides {1})'.format(k, tuple(blocks[k].stride())))
        self.rowptr = np.zeros(nb + 1, dtype=np.int32)
        for i, _ in keys:
            self.rowptr[i + 1] += 1
        np.cumsum(self.rowptr, out=self.rowptr)
        self.colidx = np.array([j for _, j in keys], dtype=np.int32)
        self.address = np.array([blocks[k].data_ptr() for k in keys], dtype=np.uint64)
        self.nb = nb

    def args(self):
        as_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        return self.nb, as_ptr(self.bounds), as_ptr(self.rowptr), as_ptr(self.colidx), as_ptr(self.address)


def _require_row_major(B, name):
    if B.dim() != 2 or (B.shape[1] > 1 and B.stride(1) != 1):
        raise ValueError('{0}: a two-dimensional tensor with a contiguous last dimension is expected (shape {1}, strides {2})'.format(
            name, tuple(B.shape), tuple(B.stride())))


def block_potrf(table, inverses, first=0, last=None):
    """In-place block Cholesky of the block rows first <= r < last (default: all; later rows are left as the Schur complement);
    returns 0 or the 1-based index of the first non-positive pivot."""
    torch = require_gpu()
    inverses, pi = _table(inverses)
    info = torch.zeros(1, dtype=torch.int32, device=device())
    _lib.call('shg_block_potrf_rows', *table.args(), pi, int(first), int(table.nb if last is None else last), _ptr(info), _stream())
    return int(info.item())


def block_potrf_pair(table0, inverses0, table1, inverses1, first=0, last=None):
    """block_potrf for two matrices of the same structure (bounds, stored blocks) in one pass, every launch serving both
    (shg_block_potrf_rows_pair); returns the two pivot flags."""
    torch = require_gpu()
    for a, b in ((table0.bounds - table0.bounds[0], table1.bounds - table1.bounds[0]), (table0.rowptr, table1.rowptr), (table0.colidx, table1.colidx)):
        if a.shape != b.shape or not np.array_equal(a, b):
            raise ValueError('block_potrf_pair: the two matrices differ in structure')
    inverses0, p0 = _table(inverses0)
    inverses1, p1 = _table(inverses1)
    info = torch.zeros(2, dtype=torch.int32, device=device())
    nb, bounds, rowptr, colidx, address0 = table0.args()
    _lib.call('shg_block_potrf_rows_pair', nb, bounds, rowptr, colidx, address0, p0, table1.args()[4], p1, int(first),
              int(table0.nb if last is None else last), _ptr(info), _stream())
    flags = info.cpu()
    return int(flags[0]), int(flags[1])


LOOKAHEAD_MODES = {False: 0, True: 1, 'off': 0, 'on': 1, 'carry': 2, 'plain': 3}


def block_set_lookahead(mode):
    """The factorisation of a diagonal block overlaps its panel steps on two more streams unless the calling THREAD turns that
    off (shg_block_set_lookahead): threads that factor several matrices at once do better without.  mode: False / 'off', True /
    'on' (chain rows carry their coupling block through the sweep when a second hardware queue was found), 'carry' (always),
    'plain' (never)."""
    _lib.call('shg_block_set_lookahead', LOOKAHEAD_MODES[mode])


def block_lookahead_info():
    """{'mode', 'side_queues_apart', 'chain_rows_carry_coupling'} of the calling thread on the current stream."""
    arr = (ctypes.c_int * 4)()
    _lib.call('shg_block_lookahead_info', _stream(), arr)
    return {'mode': int(arr[0]), 'side_queues_apart': int(arr[1]), 'chain_rows_carry_coupling': bool(arr[2])}


def block_solve(table, inverses, transpose, B):
    """B [n, k] <- W^-1 B or W^-T B in place (device tensor, contiguous last dimension)."""
    _require_row_major(B, 'block_solve')
    inverses, pi = _table(inverses)
    _lib.call('shg_block_solve', *table.args(), pi, 1 if transpose else 0, _ptr(B), B.shape[1], max(B.stride(0), 1), _stream())
    return B


def block_sparse_inverse(table, inverses):
    inverses, pi = _table(inverses)
    _lib.call('shg_block_sparse_inverse', *table.args(), pi, _stream())


def block_solve_rows(table, inverses, transpose, first, last, B):
    """block_solve restricted to the block rows first <= r < last (forward sweep: later rows receive the updates; backward sweep:
    later rows hold the solution already), in place."""
    _require_row_major(B, 'block_solve_rows')
    inverses, pi = _table(inverses)
    _lib.call('shg_block_solve_rows', *table.args(), pi, 1 if transpose else 0, int(first), int(last), _ptr(B), B.shape[1], max(B.stride(0), 1), _stream())
    return B


def block_sparse_inverse_rows(table, inverses, first, last):
    """Takahashi recursion of the block rows last - 1 .. first; the blocks of the later rows hold their entries of the inverse already."""
    inverses, pi = _table(inverses)
    _lib.call('shg_block_sparse_inverse_rows', *table.args(), pi, int(first), int(last), _stream())


def block_inverse(table, inverses):
    inverses, pi = _table(inverses)
    _lib.call('shg_block_inverse', *table.args(), pi, _stream())


def block_multiply(table, mode, B):
    """mode 0: W B, 1: the reference's W^T B (assigning form), 2: N B with the upper blocks of a symmetric N."""
    torch = require_gpu()
    _require_row_major(B, 'block_multiply')
    out = torch.empty((B.shape[0], B.shape[1]), dtype=B.dtype, device=B.device)
    _lib.call('shg_block_multiply', *table.args(), int(mode), _ptr(B), B.shape[1], max(B.stride(0), 1), _ptr(out), max(out.stride(0), 1), _stream())
    return out


def scale_columns(F, w):
    """F[:, j] *= w[j] in place (window function of Grid.window_matrix) on the device."""
    torch = require_gpu()
    F.mul_(to_device(w, F.device).reshape(1, -1))
    return F


def congruence(W, S):
    """W S W^T on the fp64 MFMA GEMM (device tensors or arrays); exactly symmetric for a symmetric S."""
    torch = require_gpu()
    W = W if isinstance(W, torch.Tensor) and W.is_cuda and W.dtype == torch.float64 and W.is_contiguous() else to_device(W)
    S = S if isinstance(S, torch.Tensor) and S.is_cuda and S.dtype == torch.float64 and S.is_contiguous() else to_device(S)
    if W.dim() != 2 or S.dim() != 2 or S.shape[0] != S.shape[1] or W.shape[1] != S.shape[0]:
        raise ValueError('congruence: W [n, k] and a square S [k, k] expected, got {0} and {1}'.format(tuple(W.shape), tuple(S.shape)))
    n, k = W.shape
    out = torch.empty((n, n), dtype=torch.float64, device=W.device)
    work = torch.empty((n, k), dtype=torch.float64, device=W.device)
    _lib.call('shg_congruence', n, k, _ptr(W), max(k, 1), _ptr(S), max(k, 1), _ptr(out), max(n, 1), _ptr(work), _stream())
    return out


def ravel(arr, min_degree, max_degree):
    """arr [B, Na+1, Na+1] device tensor -> [B, P] degree-wise."""
    torch = require_gpu()
    x = to_device(arr)
    B, na = x.shape[0], x.shape[-1] - 1
    P = (max_degree + 1) ** 2 - min_degree ** 2
    out = torch.empty((B, max(P, 0)), dtype=torch.float64, device=x.device)
    _lib.call('shg_ravel', _ptr(x), B, na, int(min_degree), int(max_degree), _ptr(out), _stream())
    return out


def unravel(vec, min_degree, max_degree):
    """vec [B, P] device tensor -> [B, nmax+1, nmax+1]."""
    torch = require_gpu()
    v = to_device(vec)
    B = v.shape[0]
    out = torch.empty((B, max_degree + 1, max_degree + 1), dtype=torch.float64, device=v.device)
    _lib.call('shg_unravel', _ptr(v), B, int(min_degree), int(max_degree), _ptr(out), _stream())
    return out


def degree_scale(anm, weights, first_degree):
    """anm [B, N+1, N+1] scaled by weights[n] for every degree n >= first_degree."""
    torch = require_gpu()
    x = to_device(anm)
    N = x.shape[-1] - 1
    w = to_device(weights)
    if w.numel() != N + 1:
        raise ValueError('weights must have max_degree + 1 entries')
    out = torch.empty_like(x)
    _lib.call('shg_degree_scale', _ptr(w), N, int(first_degree), _ptr(x), x.shape[0], _ptr(out), _stream())
    return out


def synthesis_points(max_degree, colat, lon, kn, anm):
    """Point-list synthesis: colat/lon [npts], kn [npts, N+1], anm [B, N+1, N+1] -> [B, npts]."""
    torch = require_gpu()
    th, lam, k, x = to_device(colat), to_device(lon), to_device(kn), to_device(anm)
    out = torch.empty((x.shape[0], th.numel()), dtype=torch.float64, device=x.device)
    _lib.call('shg_synthesis_points', int(max_degree), _ptr(th), _ptr(lam), _ptr(k), th.numel(), _ptr(x), x.shape[0], _ptr(out), _stream())
    return out


def covprop_points(max_degree, colat, lon, kn, cov, min_degree):
    torch = require_gpu()
    th, lam, k, c = to_device(colat), to_device(lon), to_device(kn), to_device(cov)
    out = torch.empty((th.numel(),), dtype=torch.float64, device=c.device)
    _lib.call('shg_covprop_points', int(max_degree), _ptr(th), _ptr(lam), _ptr(k), th.numel(), _ptr(c), int(min_degree), _ptr(out), _stream())
    return out


def epoch_rms(values, acc=None, count=0):
    """acc [M] (+)= sum over the epochs of values [B, M] squared (device); count > 0 finishes with sqrt(acc / count)."""
    torch = require_gpu()
    v = to_device(values)
    if v.dim() != 2 or not v.is_contiguous():
        v = v.reshape(v.shape[0], -1).contiguous()
    accumulate = acc is not None
    if acc is None:
        acc = torch.empty((v.shape[1],), dtype=torch.float64, device=v.device)
    _lib.call('shg_epoch_rms', _ptr(v), v.shape[0], v.shape[1], int(accumulate), int(count), _ptr(acc), _stream())
    return acc


def polygon_mask(points, polygons, buffers=(), buffer_value=True):
    """Point-in-polygon mask on the device (shg_basin_pip / shg_basin_buffer): a bool tensor [n] that holds the parity of the
    polygons containing a point, then `buffer_value` where a point lies in one of the buffers.  `points` is either the pair of
    per-axis tables (lat_tab [2, nlat], lon_tab [2, nlon]) of a regular grid or the host coordinates xyz [n, 3]; `polygons` and
    `buffers` are lists of (host frame, host edge table) as grates_amd.grid builds them."""
    torch = require_gpu()
    if isinstance(points, tuple):
        lat_tab, lon_tab = to_device(points[0]), to_device(points[1])
        nlat, nlon, xyz = lat_tab.shape[1], lon_tab.shape[1], None
        n = nlat * nlon
        args = (nlat, _ptr(lat_tab), nlon, _ptr(lon_tab), None)
    else:
        xyz = to_device(points)
        n = xyz.shape[0]
        args = (0, None, 0, None, _ptr(xyz))
    mask = torch.zeros((n,), dtype=torch.bool, device=device())
    if n == 0:
        return mask
    work = torch.empty((n + 1,), dtype=torch.int64, device=mask.device)
    for name, tables, last in (('shg_basin_pip', polygons, None), ('shg_basin_buffer', buffers, int(bool(buffer_value)))):
        for k, (frame, edges) in enumerate(tables):
            frame = np.ascontiguousarray(frame, dtype=np.float64)
            e = to_device(edges)
            _lib.call(name, *args, n, _host_ptr(frame), e.shape[0], _ptr(e), int(k == 0) if last is None else last, _ptr(work), _ptr(mask),
                      _stream())
    return mask


def winding_mask(edges, x, y):
    """winding number != 0 of the points (x, y) [n] for the closed polygon's edge table [k, 5] (shg_winding_number)."""
    torch = require_gpu()
    e, px, py = to_device(edges), to_device(x), to_device(y)
    mask = torch.empty((px.numel(),), dtype=torch.bool, device=px.device)
    _lib.call('shg_winding_number', e.shape[0], _ptr(e), _ptr(px), _ptr(py), px.numel(), _ptr(mask), _stream())
    return mask


def pack_masks(masks):
    """uint64 mask bits [P] (as int64) of a bool tensor [B, P], B <= 64 (shg_mask_pack)."""
    torch = require_gpu()
    m = masks.contiguous()
    bits = torch.empty((m.shape[1],), dtype=torch.int64, device=m.device)
    _lib.call('shg_mask_pack', _ptr(m), m.shape[0], m.shape[1], _ptr(bits), _stream())
    return bits


def basin_statistics(values, weights, bits, count):
    """[3, T, count] = area-weighted mean, rms and std of values [T, P] (fp64, contiguous, device) over each of the `count` masks whose
    bits pack_masks gave, with the weights [P] (shg_basin_statistics)."""
    torch = require_gpu()
    T, P = values.shape
    out = torch.empty((3, T, count), dtype=torch.float64, device=values.device)
    _lib.call('shg_basin_statistics', _ptr(values), T, P, _ptr(weights), _ptr(bits), int(count), _ptr(out), _stream())
    return out


def basin_functionals(plan, bits, count, area, min_degree):
    """F [count, (N+1)^2 - min_degree^2] (device): the area-weighted mean over each of the `count` masks whose bits pack_masks gave, of
    the plan's synthesis, as row vectors on the degree-wise coefficients (shg_basin_functionals); `area` [nlat, nlon]."""
    torch = require_gpu()
    a = to_device(area, plan.device).reshape(plan.nlat, plan.nlon)
    P = (plan.max_degree + 1) ** 2 - min_degree ** 2
    out = torch.empty((count, P), dtype=torch.float64, device=plan.device)
    with torch.cuda.device(plan.device):
        _lib.call('shg_basin_functionals', plan._handle, _ptr(bits), int(count), _ptr(a), int(min_degree), _ptr(out), _stream())
    return out


def basin_covariance(F, S):
    """F S F^T [B, B] (device) for F [B, n], B <= 64, from the upper triangle of S [n, n] only (shg_basin_covariance): exactly
    symmetric, bitwise reproducible."""
    torch = require_gpu()
    F = F if isinstance(F, torch.Tensor) and F.is_cuda and F.dtype == torch.float64 and F.is_contiguous() else to_device(F)
    S = S if isinstance(S, torch.Tensor) and S.is_cuda and S.dtype == torch.float64 and S.is_contiguous() else to_device(S)
    if F.dim() != 2 or S.dim() != 2 or S.shape[0] != S.shape[1] or F.shape[1] != S.shape[0]:
        raise ValueError('basin_covariance: F [B, n] and a square S [n, n] expected, got {0} and {1}'.format(tuple(F.shape), tuple(S.shape)))
    B, n = F.shape
    out = torch.empty((B, B), dtype=torch.float64, device=F.device)
    _lib.call('shg_basin_covariance', int(B), int(n), _ptr(F), max(int(n), 1), _ptr(S), max(int(n), 1), _ptr(out), _stream())
    return out


def check_acceleration_points(xyz, epochs):
    """The layout of the positions of an acceleration call with `epochs` fields: xyz [M, 3] (shared points, returns False) or
    [epochs, M, 3] (points per epoch, returns True); ValueError otherwise.  Looks at the shape only, nothing is moved."""
    shape = tuple(xyz.shape)
    if len(shape) == 2 and shape[1] == 3:
        return False
    if len(shape) == 3 and shape[2] == 3 and shape[0] == epochs:
        return True
    raise ValueError('positions must have shape (M, 3) or ({0}, M, 3), got {1}'.format(epochs, shape))


def _functional_points(stem, tail, max_degree, xyz, coefficients, GM, R):
    """out [B, M, *tail] of the point functional shg_<stem> (a batch) / shg_<stem>_om (an OrderMajorSeries)."""
    torch = require_gpu()
    om = isinstance(coefficients, OrderMajorSeries)
    if not om:
        coefficients = to_device(coefficients)
        if coefficients.dim() != 3 or coefficients.shape[1] != coefficients.shape[2] or coefficients.shape[1] != max_degree + 1:
            raise ValueError('coefficient batch must have shape (B, {0}, {0}), got {1}'.format(max_degree + 1, tuple(coefficients.shape)))
    elif coefficients.max_degree != max_degree:
        raise ValueError('the series holds degrees up to {0}, not {1}'.format(coefficients.max_degree, max_degree))
    B = coefficients.epochs if om else int(coefficients.shape[0])
    per_epoch = check_acceleration_points(xyz, B)
    x = to_device(xyz, coefficients.data.device if om else coefficients.device)
    M = int(x.shape[-2])
    out = torch.empty((B, M) + tail, dtype=torch.float64, device=x.device)
    layout = 1 if per_epoch else 0
    if om:
        _lib.call('shg_' + stem + '_om', int(max_degree), _ptr(x), M, layout, _ptr(coefficients.data), B, coefficients.padded_epochs,
                  float(GM), float(R), _ptr(out), _stream())
    else:
        _lib.call('shg_' + stem, int(max_degree), _ptr(x), M, layout, _ptr(coefficients), B, float(GM), float(R), _ptr(out), _stream())
    return out


def acceleration_points(max_degree, xyz, coefficients, GM, R):
    """Gravitational acceleration g [B, M, 3] (device, m/s^2) of the fields `coefficients` -- a batch [B, N+1, N+1] or an
    OrderMajorSeries, read in its own layout -- with constants GM and R at the positions xyz [M, 3] (shared by all fields) or
    [B, M, 3] (per field) (shg_acceleration_points / shg_acceleration_points_om)."""
    return _functional_points('acceleration_points', (3,), max_degree, xyz, coefficients, GM, R)


def gravitational_gradients_points(max_degree, xyz, coefficients, GM, R):
    """Gravitational gradient tensor T [B, M, 3, 3] (device, s^-2), T[b, m, c, d] = d g_c / d x_d, of the fields `coefficients` -- a
    batch [B, N+1, N+1] or an OrderMajorSeries, read in its own layout -- with constants GM and R at the positions xyz [M, 3] (shared
    by all fields) or [B, M, 3] (per field) (shg_gravitational_gradients_points / shg_gravitational_gradients_points_om)."""
    return _functional_points('gravitational_gradients_points', (3, 3), max_degree, xyz, coefficients, GM, R)


def potential_points(max_degree, xyz, coefficients, GM, R):
    """Gravitational potential V [B, M] (device, m^2/s^2) of the fields `coefficients` -- a batch [B, N+1, N+1] or an
    OrderMajorSeries, read in its own layout -- with constants GM and R at the positions xyz [M, 3] (shared by all fields) or
    [B, M, 3] (per field) (shg_potential_points / shg_potential_points_om)."""
    return _functional_points('potential_points', (), max_degree, xyz, coefficients, GM, R)


POINTS_AT_WINDOW = 16                                            # fields per point of one shg_*_points_at call


def points_at_plan(first):
    """(order, run_first, run_begin) of the window starts `first` [M] (host ints): the runs of consecutive points with one window start
    as shg_*_points_at takes them (int32: run r covers the points run_begin[r] .. run_begin[r + 1] - 1 and starts at field
    run_first[r]).  `order` is None where `first` is non-decreasing; else the stable sort of `first`, the runs are those of
    first[order], and the result of point order[i] is row i of the call's output.  Host only."""
    first = np.asarray(first)
    M = int(first.shape[0])
    order = None
    if M > 1 and bool(np.any(first[1:] < first[:-1])):
        order = np.argsort(first, kind='stable')
        first = first[order]
    if M == 0:
        return order, np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int32)
    starts = np.flatnonzero(np.concatenate(([True], first[1:] != first[:-1])))
    return order, np.ascontiguousarray(first[starts], dtype=np.int32), np.concatenate((starts, [M])).astype(np.int32)


def check_points_at(max_degree, xyz, coefficients, first, weights):
    """(M, B, W, first) of a shg_*_points_at call: positions xyz [M, 3], the fields `coefficients` (a batch [B, N+1, N+1] or an
    OrderMajorSeries of degree max_degree), window starts `first` [M] (host ints in 0 .. B - W, returned as an int64 array) and finite
    weights [M, W], W >= 1; ValueError otherwise.  Host arrays are checked on the host, before anything reaches the device."""
    M = check_positions(xyz)
    if isinstance(coefficients, OrderMajorSeries):
        if coefficients.max_degree != max_degree:
            raise ValueError('the series holds degrees up to {0}, not {1}'.format(coefficients.max_degree, max_degree))
        B = coefficients.epochs
    else:
        shape = tuple(coefficients.shape)
        if len(shape) != 3 or shape[1] != shape[2] or shape[1] != max_degree + 1:
            raise ValueError('coefficient batch must have shape (B, {0}, {0}), got {1}'.format(max_degree + 1, shape))
        B = int(shape[0])
    first = np.asarray(first)
    if first.shape != (M,) or first.dtype.kind not in 'iu':
        raise ValueError('first must be an integer array of shape ({0},), got {1} of {2}'.format(M, first.dtype, first.shape))
    first = first.astype(np.int64)
    if not hasattr(weights, 'shape'):
        weights = np.asarray(weights, dtype=np.float64)
    shape = tuple(weights.shape)
    if len(shape) != 2 or shape[0] != M or shape[1] < 1:
        raise ValueError('weights must have shape ({0}, W) with W >= 1, got {1}'.format(M, shape))
    W = int(shape[1])
    if W > B:
        raise ValueError('a window of {0} fields, but only {1} fields'.format(W, B))
    if M and (int(first.min()) < 0 or int(first.max()) > B - W):
        bad = int(np.flatnonzero((first < 0) | (first > B - W))[0])
        raise ValueError('first[{0}] is {1}, outside 0 .. {2} ({3} fields, windows of {4})'.format(bad, int(first[bad]), B - W, B, W))
    finite = bool(np.all(np.isfinite(weights))) if isinstance(weights, np.ndarray) else bool(weights.isfinite().all())
    if not finite:
        raise ValueError('weights must be finite')
    return M, B, W, first


def _functional_points_at(stem, tail, max_degree, xyz, coefficients, first, weights, GM, R):
    """out [M, *tail] of shg_<stem>_at (a batch) / shg_<stem>_at_om (an OrderMajorSeries): sum_j weights[i, j] of the functional of field
    first[i] + j at point i."""
    M, B, W, first = check_points_at(max_degree, xyz, coefficients, first, weights)
    if not (np.isfinite(GM) and np.isfinite(R) and R > 0):
        raise ValueError('GM and R must be finite and R positive, got {0} and {1}'.format(GM, R))
    torch = require_gpu()
    om = isinstance(coefficients, OrderMajorSeries)
    coef = coefficients.data if om else to_device(coefficients)
    x, w = to_device(xyz, coef.device), to_device(weights, coef.device)
    if M == 0:
        return torch.empty((0,) + tail, dtype=torch.float64, device=coef.device)
    order, run_first, run_begin = points_at_plan(first)
    if order is not None:
        index = torch.from_numpy(order).to(coef.device)
        x, w = x.index_select(0, index), w.index_select(0, index)
    fields = (_ptr(coef), B, coefficients.padded_epochs) if om else (_ptr(coef), B)
    out = None
    for j0 in range(0, W, POINTS_AT_WINDOW):                      # windows above 16 fields: calls of at most 16, added in order
        count = min(POINTS_AT_WINDOW, W - j0)
        part = torch.empty((M,) + tail, dtype=torch.float64, device=coef.device)
        w_part = w if count == W else w[:, j0:j0 + count].contiguous()
        shifted = np.ascontiguousarray(run_first + j0, dtype=np.int32)
        _lib.call('shg_' + stem + ('_at_om' if om else '_at'), int(max_degree), _ptr(x), M, *fields, _host_ptr(shifted), _host_ptr(run_begin),
                  int(run_first.shape[0]), _ptr(w_part), count, float(GM), float(R), _ptr(part), _stream())
        out = part if out is None else out.add_(part)
    if order is not None:
        out = torch.empty_like(out).index_copy_(0, index, out)
    return out


def acceleration_points_at(max_degree, xyz, coefficients, first, weights, GM, R):
    """Gravitational acceleration g [M, 3] (device, m/s^2) of a time-variable field, every point at its own epoch:
    g[i] = sum_{j < W} weights[i, j] g(field first[i] + j)(xyz[i]) of the fields `coefficients` -- a batch [B, N+1, N+1] or an
    OrderMajorSeries, read in its own layout -- with constants GM and R (shg_acceleration_points_at / _om).  xyz [M, 3] and weights
    [M, W] on the host or on the device; first [M] host ints, the window start per point.  Where first is not non-decreasing the points
    are reordered by a stable sort and the results scattered back; W > 16 takes one call per 16 fields, added in order."""
    return _functional_points_at('acceleration_points', (3,), max_degree, xyz, coefficients, first, weights, GM, R)


def gravitational_gradients_points_at(max_degree, xyz, coefficients, first, weights, GM, R):
    """Gravitational gradient tensor T [M, 3, 3] (device, s^-2) of a time-variable field, every point at its own epoch: as
    acceleration_points_at (shg_gravitational_gradients_points_at / _om)."""
    return _functional_points_at('gravitational_gradients_points', (3, 3), max_degree, xyz, coefficients, first, weights, GM, R)


def potential_points_at(max_degree, xyz, coefficients, first, weights, GM, R):
    """Gravitational potential V [M] (device, m^2/s^2) of a time-variable field, every point at its own epoch: as
    acceleration_points_at (shg_potential_points_at / _om)."""
    return _functional_points_at('potential_points', (), max_degree, xyz, coefficients, first, weights, GM, R)


def points_at_set_workspace_limit(nbytes):
    """The bytes of combined coefficients one launch group of the shg_*_points_at calls may hold, process-wide (0: the default of
    256 MB).  Host only."""
    _lib.call('shg_points_at_set_workspace_limit', int(nbytes))


def check_observation_weights(weights, points, components=3):
    """The layout of the weights of `points` observed positions with `components` observed values each: None (returns 0), w [M] per
    point (1) or w [M, components] per component (2), finite and >= 0; ValueError otherwise.  Host arrays are checked on the host,
    before anything reaches the device."""
    if weights is None:
        return 0
    shape = tuple(weights.shape)
    if shape != (points,) and shape != (points, components):
        raise ValueError('weights must have shape ({0},) or ({0}, {1}), got {2}'.format(points, components, shape))
    if isinstance(weights, np.ndarray):
        valid = bool(np.all(np.isfinite(weights) & (weights >= 0)))
    else:
        valid = bool((weights.isfinite() & (weights >= 0)).all())
    if not valid:
        raise ValueError('weights must be finite and not negative')
    return len(shape)


def check_degrees(min_degree, max_degree):
    """(min_degree, max_degree) as ints, 0 <= min_degree <= max_degree; ValueError otherwise."""
    min_degree, max_degree = int(min_degree), int(max_degree)
    if min_degree < 0 or min_degree > max_degree:
        raise ValueError('min_degree {0} must lie between 0 and max_degree {1}'.format(min_degree, max_degree))
    return min_degree, max_degree


def check_positions(xyz, name='positions'):
    """The number of points M of `name` [M, 3]; ValueError for another shape."""
    if len(xyz.shape) != 2 or xyz.shape[1] != 3:
        raise ValueError('{0} must have shape (M, 3), got {1}'.format(name, tuple(xyz.shape)))
    return int(xyz.shape[0])


def _design_output(max_degree, min_degree, x, *components):
    """(M, At): the number of positions x [M, 3] and the empty transposed design matrix At [P, *components, M] on their device."""
    torch = require_gpu()
    M = int(x.shape[0])
    return M, torch.empty(((max_degree + 1) ** 2 - min_degree ** 2,) + components + (M,), dtype=torch.float64, device=x.device)


def acceleration_design(max_degree, xyz, GM, R, min_degree=0, weights=None):
    """Transposed design matrix At [P, 3, M] (device) of the gravitational acceleration at the positions xyz [M, 3]: At[p, c, i] is the
    derivative of component c of g at point i with respect to coefficient p of utilities.ravel_coefficients(., min_degree, max_degree),
    P = (max_degree + 1)^2 - min_degree^2 (shg_acceleration_design).  weights [M] or [M, 3] scale the entries by sqrt(w)."""
    return _design('accelerations', dict(xyz=xyz, weights=weights), Band(*check_degrees(min_degree, max_degree), GM, R))


def acceleration_design_checked(max_degree, min_degree, x, weights, GM, R):
    """shg_acceleration_design on device tensors that acceleration_design (or NormalEquations.from_accelerations, once for all its
    blocks) has checked: positions x [M, 3], weights [M], [M, 3] or None."""
    M, out = _design_output(max_degree, min_degree, x, 3)
    _lib.call('shg_acceleration_design', max_degree, min_degree, _ptr(x), M, None if weights is None else _ptr(weights),
              0 if weights is None else weights.dim(), float(GM), float(R), _ptr(out), M, _stream())
    return out


GRADIENT_COMPONENTS = ('xx', 'xy', 'xz', 'yy', 'yz', 'zz')       # canonical order: bit j of shg_gradient_design's component set
FRAME_TOLERANCE = 1e-12                                          # |F F^T - I| of an instrument frame


def gradient_components(components):
    """The positions in GRADIENT_COMPONENTS of the selected tensor components, ascending: `components` is a sequence of distinct
    names in any order, None for all six; ValueError otherwise."""
    if components is None:
        return list(range(6))
    names = [components] if isinstance(components, str) else list(components)
    unknown = [name for name in names if name not in GRADIENT_COMPONENTS]
    if unknown:
        raise ValueError('unknown gradient component {0!r}: expected names from {1}'.format(unknown[0], GRADIENT_COMPONENTS))
    if len(set(names)) != len(names):
        raise ValueError('gradient components must be distinct, got {0}'.format(tuple(names)))
    if not names:
        raise ValueError('at least one gradient component expected')
    return sorted(GRADIENT_COMPONENTS.index(name) for name in names)


def check_frames(frames, points):
    """Instrument frames [M, 3, 3] (row a: axis a in Earth-fixed coordinates) must have orthonormal rows, |F F^T - I| <=
    FRAME_TOLERANCE: host arrays are checked on the host, device tensors by one reduction on the device; ValueError otherwise."""
    shape = tuple(frames.shape)
    if shape != (points, 3, 3):
        raise ValueError('frames must have shape ({0}, 3, 3), got {1}'.format(points, shape))
    if points == 0:
        return
    if isinstance(frames, np.ndarray):
        defect = float(np.abs(np.einsum('iac,ibc->iab', frames, frames) - np.eye(3)).max())
    else:
        torch = require_gpu()
        eye = torch.eye(3, dtype=frames.dtype, device=frames.device)
        defect = float((frames @ frames.transpose(1, 2) - eye).abs().max().item())
    if not defect <= FRAME_TOLERANCE:
        raise ValueError('frames must have orthonormal rows: |F F^T - I| is {0:.3g}, above {1:g}'.format(defect, FRAME_TOLERANCE))


def gradient_design(max_degree, xyz, GM, R, min_degree=0, frames=None, components=None, weights=None):
    """Transposed design matrix At [P, K, M] (device) of the gravitational gradient tensor at the positions xyz [M, 3]: At[p, k, i] is
    the derivative of the k-th selected component of T' = F T F^T at point i with respect to coefficient p of
    utilities.ravel_coefficients(., min_degree, max_degree) (shg_gradient_design).  frames [M, 3, 3] hold the instrument axes as rows
    (None: the Earth-fixed tensor); components is a sequence of distinct names from GRADIENT_COMPONENTS in any order (None: all six),
    the output always in canonical order; weights [M] or [M, K] scale the entries by sqrt(w)."""
    return _design('gradients', dict(xyz=xyz, frames=frames, components=components, weights=weights),
                   Band(*check_degrees(min_degree, max_degree), GM, R))


def gradient_design_checked(max_degree, min_degree, x, frames, picked, weights, GM, R):
    """shg_gradient_design on device tensors that gradient_design (or NormalEquations.from_gradients, once for all its blocks) has
    checked: positions x [M, 3], frames [M, 3, 3] or None, the ascending component positions `picked`, weights [M], [M, K] or None."""
    M, out = _design_output(max_degree, min_degree, x, len(picked))
    _lib.call('shg_gradient_design', max_degree, min_degree, _ptr(x), M, None if frames is None else _ptr(frames), sum(1 << j for j in picked),
              None if weights is None else _ptr(weights), 0 if weights is None else weights.dim(), float(GM), float(R), _ptr(out), M, _stream())
    return out


def check_pair_positions(xyz_a, xyz_b):
    """The positions of M satellite pairs, xyz_a [M, 3] and xyz_b [M, 3]: returns M; ValueError otherwise.  Looks at the shapes only."""
    M, second = check_positions(xyz_a, 'positions of the first satellite'), check_positions(xyz_b, 'positions of the second satellite')
    if M != second:
        raise ValueError('{0} positions of the first satellite but {1} of the second'.format(M, second))
    return M


def check_directions(directions, M):
    """Lines of sight [M, 3] must be finite and of unit length, | |e| - 1 | <= FRAME_TOLERANCE: host arrays are checked on the host,
    device tensors by one reduction on the device; ValueError otherwise."""
    shape = tuple(directions.shape)
    if shape != (M, 3):
        raise ValueError('directions must have shape ({0}, 3), got {1}'.format(M, shape))
    if M == 0:
        return
    if isinstance(directions, np.ndarray):
        defect = float(np.abs(np.sqrt(np.sum(directions * directions, axis=1)) - 1.0).max())
    else:
        defect = float(((directions * directions).sum(dim=1).sqrt() - 1.0).abs().max().item())
    if not defect <= FRAME_TOLERANCE:                                # a NaN or an infinity anywhere makes the defect NaN or inf
        raise ValueError('directions must be finite unit vectors: | |e| - 1 | is {0:.3g}, above {1:g}'.format(defect, FRAME_TOLERANCE))


def check_pairs_apart(xyz_a, xyz_b):
    """No pair may coincide where the line of sight comes from the positions (a == b has none): host arrays are checked on the host,
    device tensors by one reduction on the device; ValueError otherwise."""
    if int(xyz_a.shape[0]) == 0:
        return
    if isinstance(xyz_a, np.ndarray) and isinstance(xyz_b, np.ndarray):
        count = int(np.count_nonzero(np.all(xyz_a == xyz_b, axis=1)))
    else:
        a = to_device(xyz_a)
        count = int((a == to_device(xyz_b, a.device)).all(dim=1).sum().item())
    if count:
        raise ValueError('{0} pairs have both satellites at the same position: their line of sight is undefined, pass directions'.format(count))


def los_design(max_degree, xyz_a, xyz_b, GM, R, min_degree=0, directions=None, weights=None):
    """Transposed design matrix At [P, M] (device) of the line-of-sight gravity difference of the satellite pairs xyz_a [M, 3],
    xyz_b [M, 3]: At[p, i] is the derivative of e_i . (g(b_i) - g(a_i)) with respect to coefficient p of
    utilities.ravel_coefficients(., min_degree, max_degree), P = (max_degree + 1)^2 - min_degree^2 (shg_los_design).  directions
    [M, 3] are the lines of sight e (unit vectors; None: (b - a) / |b - a|, and no pair may then coincide); weights [M] scale the
    entries by sqrt(w)."""
    return _design('line_of_sight', dict(xyz_a=xyz_a, xyz_b=xyz_b, directions=directions, weights=weights),
                   Band(*check_degrees(min_degree, max_degree), GM, R))


def los_design_checked(max_degree, min_degree, a, b, directions, weights, GM, R):
    """shg_los_design on device tensors that los_design (or NormalEquations.from_line_of_sight, once for all its blocks) has checked:
    positions a, b [M, 3], directions [M, 3] or None, weights [M] or None."""
    M, out = _design_output(max_degree, min_degree, a)
    _lib.call('shg_los_design', max_degree, min_degree, _ptr(a), _ptr(b), None if directions is None else _ptr(directions), M,
              None if weights is None else _ptr(weights), float(GM), float(R), _ptr(out), M, _stream())
    return out


def los_design_pass(max_degree):
    """Pairs per pass of shg_los_design at this degree: the solid harmonics of both satellites share the 256 MB of a pass of the
    acceleration's design matrix (host only, no HIP call)."""
    count = _lib.load().shg_los_design_pass(int(max_degree))
    if count < 0:
        raise ValueError('max_degree {0} is out of range'.format(max_degree))
    return count


def check_point_weights(weights, M):
    """Weights of observations with one value per point (pair): None (returns 0) or w [M], finite and >= 0 (returns 1); ValueError
    otherwise."""
    layout = check_observation_weights(weights, M, 1)
    if layout and len(weights.shape) != 1:
        raise ValueError('weights must have shape ({0},), got {1}'.format(M, tuple(weights.shape)))
    return layout


def potential_design(max_degree, xyz, GM, R, min_degree=0, weights=None):
    """Transposed design matrix At [P, M] (device) of the gravitational potential at the positions xyz [M, 3]: At[p, i] is the
    derivative of V at point i with respect to coefficient p of utilities.ravel_coefficients(., min_degree, max_degree),
    P = (max_degree + 1)^2 - min_degree^2 (shg_potential_design).  weights [M] scale the entries by sqrt(w)."""
    return _design('potentials', dict(xyz=xyz, weights=weights), Band(*check_degrees(min_degree, max_degree), GM, R))


def potential_design_checked(max_degree, min_degree, x, weights, GM, R):
    """shg_potential_design on device tensors that potential_design (or NormalEquations.from_potentials, once for all its blocks) has
    checked: positions x [M, 3], weights [M] or None."""
    M, out = _design_output(max_degree, min_degree, x)
    _lib.call('shg_potential_design', max_degree, min_degree, _ptr(x), M, None if weights is None else _ptr(weights), float(GM), float(R), _ptr(out),
              M, _stream())
    return out


def potential_difference_design(max_degree, xyz_a, xyz_b, GM, R, min_degree=0, weights=None):
    """Transposed design matrix At [P, M] (device) of the potential difference of the satellite pairs xyz_a [M, 3], xyz_b [M, 3]:
    At[p, i] is the derivative of V(b_i) - V(a_i) with respect to coefficient p of utilities.ravel_coefficients(., min_degree,
    max_degree) (shg_potential_difference_design).  A pair with a == b is legal and gives a zero column; weights [M] scale the entries
    by sqrt(w)."""
    return _design('potential_differences', dict(xyz_a=xyz_a, xyz_b=xyz_b, weights=weights), Band(*check_degrees(min_degree, max_degree), GM, R))


def potential_difference_design_checked(max_degree, min_degree, a, b, weights, GM, R):
    """shg_potential_difference_design on device tensors that potential_difference_design (or
    NormalEquations.from_potential_differences, once for all its blocks) has checked: positions a, b [M, 3], weights [M] or None."""
    M, out = _design_output(max_degree, min_degree, a)
    _lib.call('shg_potential_difference_design', max_degree, min_degree, _ptr(a), _ptr(b), M, None if weights is None else _ptr(weights), float(GM),
              float(R), _ptr(out), M, _stream())
    return out


RBF_KINDS = ('acceleration', 'line_of_sight', 'potential', 'potential_difference')      # position: the kind of shg_rbf_design


def rbf_design_info():
    """(nodes per workgroup, nodes a lane runs side by side, points per workgroup, most nodes of one call) of shg_rbf_design: the seams
    of its launch geometry (host only, no HIP call)."""
    arr = (ctypes.c_int * 4)()
    _lib.call('shg_rbf_design_info', arr)
    return tuple(int(v) for v in arr)


def rbf_node_table(basis):
    """What shg_rbf_design reads of a gravityfield.RadialBasisFunctions, built on the host once per basis and kept on it: the degree
    factors k_n [N + 1] (host; ValueError for an anisotropic K) and the nodes [J, 4] on the device, the unit vector of (geocentric
    colatitude, longitude) of every nodal point on the ellipsoid of its point distribution and R / r_j.  The table follows the nodal
    points at the time of the first call: a basis whose points change afterwards is a new basis (copy())."""
    cached = getattr(basis, '_rbf_node_table', None)
    if cached is None or cached[2] != float(basis.R):
        from . import utilities
        points = basis.point_distribution
        shape = np.ascontiguousarray(basis.degree_factors, dtype=np.float64)
        colat = utilities.colatitude(points.latitude, points.semimajor_axis, points.flattening)
        radius = utilities.geocentric_radius(points.latitude, points.semimajor_axis, points.flattening)
        lon = np.asarray(points.longitude, dtype=np.float64)
        nodes = np.stack((np.sin(colat) * np.cos(lon), np.sin(colat) * np.sin(lon), np.cos(colat), basis.R / radius), axis=1)
        cached = basis._rbf_node_table = (shape, to_device(np.ascontiguousarray(nodes.reshape(-1, 4))), float(basis.R))
    return cached[:2]


def _rbf_design_output(basis, x, *components):
    """(shape, nodes, J, M, At): the node table of the basis (rbf_node_table) with the nodes on the device of the positions x [M, 3],
    the numbers of nodes and positions and the empty transposed design matrix At [J, *components, M] on that device."""
    torch = require_gpu()
    shape, nodes = rbf_node_table(basis)
    if nodes.device != x.device:
        nodes = nodes.to(x.device)
    J, M = int(nodes.shape[0]), int(x.shape[0])
    return shape, nodes, J, M, torch.empty((J,) + components + (M,), dtype=torch.float64, device=x.device)


def rbf_design(kind, basis, xyz, xyz_b=None, directions=None, weights=None):
    """Transposed design matrix At [J, K, M] (acceleration, K = 3) or [J, M] (device) of the observations `kind` (one of RBF_KINDS) with
    respect to the node values of the isotropic gravityfield.RadialBasisFunctions `basis`: At[j, ..., i] is the derivative of the
    observation at point (pair) i with respect to value j (shg_rbf_design).  xyz [M, 3] are the points, or the first satellites of the
    pair kinds, whose second satellites are xyz_b [M, 3]; directions [M, 3] are the lines of sight of 'line_of_sight' (None:
    (b - a) / |b - a|, and no pair may then coincide); weights [M] (or [M, 3], acceleration only) scale the entries by sqrt(w).  The
    columns equal those of the spherical harmonic design matrix of the basis's band times basis.to_potential_coefficients_matrix()."""
    if kind not in RBF_KINDS:
        raise ValueError('unknown kind {0!r}: expected one of {1}'.format(kind, RBF_KINDS))
    entry = OBSERVATION_KINDS[RBF_OBSERVATION_KINDS[kind]]
    if 'xyz_b' in entry.points and xyz_b is None:
        raise ValueError('{0} needs the positions of the second satellite'.format(kind))
    given = dict(xyz=xyz, xyz_a=xyz, xyz_b=xyz_b, directions=directions, weights=weights)
    return _design(RBF_OBSERVATION_KINDS[kind], {name: given[name] for name in entry.points + ('weights',) if name != entry.observed}, basis_band(basis))


def rbf_design_checked(kind, basis, a, b, directions, weights):
    """shg_rbf_design on device tensors that rbf_design (or a RadialBasisParameters.from_* or of_*, once for all its blocks) has checked:
    positions a [M, 3], b [M, 3] or None, directions [M, 3] or None, weights [M], [M, 3] or None."""
    shape, nodes, J, M, out = _rbf_design_output(basis, a, *((3,) if kind == 'acceleration' else ()))
    _lib.call('shg_rbf_design', RBF_KINDS.index(kind), int(basis.max_degree), int(basis.min_degree), _host_ptr(shape), _ptr(nodes), J, _ptr(a),
              None if b is None else _ptr(b), None if directions is None else _ptr(directions), M, None if weights is None else _ptr(weights),
              0 if weights is None else weights.dim(), float(basis.GM), float(basis.R), _ptr(out), M, _stream())
    return out


def rbf_gradient_design(basis, xyz, frames=None, components=None, weights=None):
    """Transposed design matrix At [J, K, M] (device) of the gravitational gradient tensor at the positions xyz [M, 3] with respect to
    the node values of the isotropic gravityfield.RadialBasisFunctions `basis`: At[j, k, i] is the derivative of the k-th selected
    component of T' = F T F^T at point i with respect to value j (shg_rbf_gradient_design).  frames, components and weights as in
    gradient_design: frames [M, 3, 3] hold the instrument axes as rows (None: the Earth-fixed tensor), components is a sequence of
    distinct names from GRADIENT_COMPONENTS (None: all six), the output always in canonical order, weights [M] or [M, K] scale the
    entries by sqrt(w).  The columns equal those of gradient_design of the basis's band times
    basis.to_potential_coefficients_matrix()."""
    return _design('gradients', dict(xyz=xyz, frames=frames, components=components, weights=weights), basis_band(basis))


def rbf_gradient_design_checked(basis, x, frames, picked, weights):
    """shg_rbf_gradient_design on device tensors that rbf_gradient_design (or RadialBasisParameters.from_gradients, once for all its
    blocks) has checked: positions x [M, 3], frames [M, 3, 3] or None, the ascending component positions `picked`, weights [M], [M, K]
    or None."""
    shape, nodes, J, M, out = _rbf_design_output(basis, x, len(picked))
    _lib.call('shg_rbf_gradient_design', int(basis.max_degree), int(basis.min_degree), _host_ptr(shape), _ptr(nodes), J, _ptr(x), M,
              None if frames is None else _ptr(frames), sum(1 << j for j in picked), None if weights is None else _ptr(weights),
              0 if weights is None else weights.dim(), float(basis.GM), float(basis.R), _ptr(out), M, _stream())
    return out


# ---- the kinds of observation: what the *_design functions above and every from_* and of_* of lstsq know of a kind, stated once ---------
Band = collections.namedtuple('Band', 'min_degree max_degree GM R basis', defaults=(None,))
Band.__doc__ = """The parameters of a design call: the coefficients of degrees min_degree .. max_degree with the constants GM and R, or the
node values of the isotropic gravityfield.RadialBasisFunctions `basis` (None: the coefficients)."""

ObservationKind = collections.namedtuple('ObservationKind', 'points observed options check values design rbf_design')
ObservationKind.__doc__ = """One kind of observation.  points: its per-point arguments in call order (weights [M] or [M, K], which every
kind takes, come after them); the first decides whether results are host arrays or device tensors, `observed` names the one that holds
the observed values, which the *_design functions do not take.  options: its per-call arguments.  check(arguments) runs the host checks
of the kind on the dict of a call, in a fixed order, and returns (M, K, the layout of the weights, extra), extra being what the design
call needs beyond the tensors; the shape of the observed values is checked only where the dict holds them: before the weights, and
for gradients behind the components, which give K.  values(l, extra): the observed values on the device as l [M, K].  design(band,
tensors, extra) and rbf_design(band, tensors, extra): the transposed design matrix [P, K, Mb] or [P, Mb] with respect to the
coefficients, and to the node values of band.basis, of a slice of the per-point tensors and the weights, on the device and checked."""


def basis_band(basis):
    """the Band of the node values of a gravityfield.RadialBasisFunctions"""
    return Band(basis.min_degree, basis.max_degree, basis.GM, basis.R, basis)


def _check_scalar_observations(arguments, name, M, unit):
    """one observed value per point (pair), where the call holds them: `name` [M]"""
    if name in arguments:
        values = arguments[name]
        if len(values.shape) != 1:
            raise ValueError('{0} must have shape (M,), got {1}'.format(name, tuple(values.shape)))
        if int(values.shape[0]) != M:
            raise ValueError('{0} {1} but {2} {3}'.format(M, unit, int(values.shape[0]), name))


def _check_accelerations(a):
    M = check_positions(a['xyz'])
    if 'g' in a and check_positions(a['g'], 'accelerations') != M:
        raise ValueError('{0} positions but {1} accelerations'.format(M, int(a['g'].shape[0])))
    return M, 3, check_observation_weights(a['weights'], M), None


def _check_gradients(a):
    M = check_positions(a['xyz'])
    picked = gradient_components(a['components'])
    K, full = len(picked), False
    if 'gradients' in a:
        shape = tuple(a['gradients'].shape)
        full = len(shape) == 3 and shape[1:] == (3, 3)
        if not full and (len(shape) != 2 or shape[1] != K):
            raise ValueError('gradients must have shape (M, {0}) or (M, 3, 3), got {1}'.format(K, shape))
        if shape[0] != M:
            raise ValueError('{0} positions but {1} gradients'.format(M, shape[0]))
    layout = check_observation_weights(a['weights'], M, K)
    if a['frames'] is not None:
        check_frames(a['frames'], M)
    return M, K, layout, (picked, full)


def _check_line_of_sight(a):
    M = check_pair_positions(a['xyz_a'], a['xyz_b'])
    _check_scalar_observations(a, 'differences', M, 'pairs')
    layout = check_point_weights(a['weights'], M)
    if a['directions'] is not None:
        check_directions(a['directions'], M)
    else:
        check_pairs_apart(a['xyz_a'], a['xyz_b'])
    return M, 1, layout, None


def _check_potentials(a):
    M = check_positions(a['xyz'])
    _check_scalar_observations(a, 'potentials', M, 'positions')
    return M, 1, check_point_weights(a['weights'], M), None


def _check_potential_differences(a):
    M = check_pair_positions(a['xyz_a'], a['xyz_b'])
    _check_scalar_observations(a, 'differences', M, 'pairs')
    return M, 1, check_point_weights(a['weights'], M), None


def _picked_entries(l, extra):
    """the selected upper-triangle entries of gradients given as [M, 3, 3]"""
    picked, full = extra
    return l.reshape(int(l.shape[0]), 9)[:, [(0, 1, 2, 4, 5, 8)[i] for i in picked]] if full else l


def _one_column(l, extra):
    return l.reshape(-1, 1)


def _rbf_call(kind):
    """the design call of a kind of RBF_KINDS on the tensors of a table entry"""
    first = 'xyz_a' if kind in ('line_of_sight', 'potential_difference') else 'xyz'
    return lambda band, t, extra: rbf_design_checked(kind, band.basis, t[first], t.get('xyz_b'), t.get('directions'), t['weights'])


OBSERVATION_KINDS = {
    'accelerations': ObservationKind(
        ('xyz', 'g'), 'g', (), _check_accelerations, lambda l, extra: l,
        lambda band, t, extra: acceleration_design_checked(band.max_degree, band.min_degree, t['xyz'], t['weights'], band.GM, band.R),
        _rbf_call('acceleration')),
    'gradients': ObservationKind(
        ('xyz', 'gradients', 'frames'), 'gradients', ('components',), _check_gradients, _picked_entries,
        lambda band, t, extra: gradient_design_checked(band.max_degree, band.min_degree, t['xyz'], t['frames'], extra[0], t['weights'], band.GM, band.R),
        lambda band, t, extra: rbf_gradient_design_checked(band.basis, t['xyz'], t['frames'], extra[0], t['weights'])),
    'line_of_sight': ObservationKind(
        ('xyz_a', 'xyz_b', 'differences', 'directions'), 'differences', (), _check_line_of_sight, _one_column,
        lambda band, t, extra: los_design_checked(band.max_degree, band.min_degree, t['xyz_a'], t['xyz_b'], t['directions'], t['weights'], band.GM, band.R),
        _rbf_call('line_of_sight')),
    'potentials': ObservationKind(
        ('xyz', 'potentials'), 'potentials', (), _check_potentials, _one_column,
        lambda band, t, extra: potential_design_checked(band.max_degree, band.min_degree, t['xyz'], t['weights'], band.GM, band.R),
        _rbf_call('potential')),
    'potential_differences': ObservationKind(
        ('xyz_a', 'xyz_b', 'differences'), 'differences', (), _check_potential_differences, _one_column,
        lambda band, t, extra: potential_difference_design_checked(band.max_degree, band.min_degree, t['xyz_a'], t['xyz_b'], t['weights'], band.GM, band.R),
        _rbf_call('potential_difference')),
}
RBF_OBSERVATION_KINDS = dict(zip(RBF_KINDS, ('accelerations', 'line_of_sight', 'potentials', 'potential_differences')))      # the table's names


def upload_observations(kind, arguments):
    """The per-point arguments and the weights of a checked call as device tensors, {name: tensor or None}: the first on the current
    device, the others where it is.  An argument the call does not hold (the observed values, for the *_design functions) is left out."""
    first = to_device(arguments[kind.points[0]])
    tensors = {kind.points[0]: first}
    for name in kind.points[1:] + ('weights',):
        if name in arguments:
            tensors[name] = None if arguments[name] is None else to_device(arguments[name], first.device)
    return tensors


def _design(kind, arguments, band):
    """The public *_design functions behind check_degrees: the checks of the kind on the host, an anisotropic basis refused before
    anything else reaches the device, then the design call on the uploaded arguments."""
    kind = OBSERVATION_KINDS[kind]
    extra = kind.check(arguments)[3]
    if band.basis is not None:
        rbf_node_table(band.basis)
    return (kind.design if band.basis is None else kind.rbf_design)(band, upload_observations(kind, arguments), extra)


def rbf_surface_info():
    """(nodes per workgroup, nodes a lane runs side by side, points per workgroup, most nodes of one call) of shg_rbf_surface: the seams
    of its launch geometry (host only, no HIP call)."""
    arr = (ctypes.c_int * 4)()
    _lib.call('shg_rbf_surface_info', arr)
    return tuple(int(v) for v in arr)


def rbf_surface_tables(grid, kernel, basis):
    """(points [M, 3], kn_t [N + 1, M]) on the device: what shg_rbf_surface reads of the M points of `grid` for the functional `kernel`
    (a name of kernel.get_kernel) and the band and constants of the gravityfield.RadialBasisFunctions `basis`.  points are the unit
    vectors of (geocentric colatitude, longitude) of the grid points on the grid's ellipsoid; kn_t is gravityfield.surface_factors with
    GM and R of the basis, degree-major -- the colatitudes and factors the spherical harmonic route of the grid uses, bit for bit --
    with the rows below basis.min_degree set to zero on the host.  The pair is cached by content like the point tables of to_grid
    (cached_point_tables: the factors of 25600 points at d/o 60 are 10 ms of NumPy, more than the kernels of a map need): callers read
    the tensors and do not write to them."""
    def build():
        colat, lon, kn = grid._point_tables(kernel, int(basis.max_degree), basis.GM, basis.R)
        lon = np.asarray(lon, dtype=np.float64)
        kn_t = np.ascontiguousarray(np.asarray(kn, dtype=np.float64).T)
        kn_t[:int(basis.min_degree)] = 0.0
        return np.stack((np.sin(colat) * np.cos(lon), np.sin(colat) * np.sin(lon), np.cos(colat)), axis=1), kn_t
    tag = ('rbf_surface', str(kernel), int(basis.min_degree), float(basis.GM), float(basis.R), float(grid.semimajor_axis), float(grid.flattening))
    return cached_point_tables(int(basis.max_degree), grid.latitude, grid.longitude, tag, build)


def _rows_of_doubles(t, name):
    """the row stride of a float64 device tensor [rows, columns] whose last dimension is contiguous"""
    torch = require_gpu()
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1)):
        raise ValueError('{0} must be a two-dimensional float64 device tensor with a contiguous last dimension'.format(name))
    return max(int(t.stride(0)), int(t.shape[1]), 1) if t.shape[0] > 1 else max(int(t.shape[1]), 1)


def rbf_surface(basis, points, kn_t):
    """Transposed surface synthesis matrix St [J, M] (device) of the isotropic gravityfield.RadialBasisFunctions `basis` at the points
    of rbf_surface_tables (or a block of them: points[a:b] and kn_t[:, a:b], whose row stride is honoured): St[j, i] is the value at
    point i for a unit value at node j (shg_rbf_surface).  The columns of St^T equal those of the grid's synthesis matrix of the
    basis's band times basis.to_potential_coefficients_matrix()."""
    torch = require_gpu()
    shape, nodes = rbf_node_table(basis)
    ldk = _rows_of_doubles(kn_t, 'kn_t')
    if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.float64 and points.dim() == 2 and points.shape[1] == 3
            and points.is_contiguous()):
        raise ValueError('points must be a contiguous float64 device tensor of shape (M, 3)')
    J, M = int(nodes.shape[0]), int(points.shape[0])
    if tuple(kn_t.shape) != (int(basis.max_degree) + 1, M):
        raise ValueError('kn_t of shape {0} does not hold degrees 0 .. {1} of {2} points'.format(tuple(kn_t.shape), int(basis.max_degree), M))
    if nodes.device != points.device:
        nodes = nodes.to(points.device)
    out = torch.empty((J, M), dtype=torch.float64, device=points.device)
    _lib.call('shg_rbf_surface', int(basis.max_degree), int(basis.min_degree), _host_ptr(shape), _ptr(nodes), J, _ptr(points), _ptr(kn_t), ldk, M,
              _ptr(out), M, _stream())
    return out


def column_dots(X, Y):
    """out [cols] (device) with out[i] = sum_r X[r, i] Y[r, i] for float64 device tensors X, Y [rows, cols] (row strides are honoured):
    the diagonal of X^T Y without the product (shg_column_dots).  The order of the sum depends on the number of rows alone: a column
    gives the same bits in any batch, at any position and in every call."""
    torch = require_gpu()
    ldx, ldy = _rows_of_doubles(X, 'X'), _rows_of_doubles(Y, 'Y')
    if tuple(X.shape) != tuple(Y.shape) or X.device != Y.device:
        raise ValueError('column_dots: X {0} and Y {1} must have one shape and one device'.format(tuple(X.shape), tuple(Y.shape)))
    rows, cols = int(X.shape[0]), int(X.shape[1])
    out = torch.empty((cols,), dtype=torch.float64, device=X.device)
    _lib.call('shg_column_dots', rows, cols, _ptr(X), ldx, _ptr(Y), ldy, _ptr(out), _stream())
    return out


def leverages(Ui, X, out=None):
    """out [cols] (device) with out[j] = |Ui^T x_j|^2 for the columns x_j of the float64 device tensor X [n, cols] and the upper
    triangular Ui [n, n] = U^-1 of a Cholesky factor N = U^T U, as trtri returns it: x_j^T N^-1 x_j, the leverage of the
    observation whose whitened, weighted row of the design matrix is x_j (shg_leverages).  Ui^T X is formed on the fp64 MFMA and
    never stored; what Ui holds below its diagonal is not used.  Row strides are honoured.  An entry depends on n, Ui and its own
    column only: a column gives the same bits alone, in any batch, at any position and in every call.  out: a contiguous float64
    device vector [cols] to write to (default: a new one)."""
    torch = require_gpu()
    for t, name in ((Ui, 'Ui'), (X, 'X')):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 2):
            raise ValueError('leverages: {0} must be a two-dimensional float64 device tensor'.format(name))
    ldu, ldx = _rows_of_doubles(Ui, 'Ui'), _rows_of_doubles(X, 'X')
    n, cols = int(X.shape[0]), int(X.shape[1])
    if tuple(Ui.shape) != (n, n) or Ui.device != X.device:
        raise ValueError('leverages: Ui {0} must be ({1}, {1}) on the device of X'.format(tuple(Ui.shape), n))
    if out is None:
        out = torch.empty((cols,), dtype=torch.float64, device=X.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (cols,) and out.is_contiguous()
              and out.device == X.device):
        raise ValueError('leverages: out must be a contiguous float64 device vector of {0} entries'.format(cols))
    else:
        Plan._written(out)
    _lib.call('shg_leverages', n, cols, _ptr(Ui), ldu, _ptr(X), ldx, _ptr(out), _stream())
    return out


WHITEN_ROWS_ORDER = 128        # the longest filter of shg_whiten_rows; above it whiten_rows calls shg_whiten_rows_long


def _rows_view(t, width):
    """(tensor, leading dimension) of t as rows of `width` columns: t itself where it is two-dimensional with unit stride along its rows
    (dense, or a column slice of a wider matrix), else a dense copy"""
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= width:
        return t, int(t.stride(0))
    return t.contiguous(), width


def _row_count(lead):
    """the rows of a tensor whose leading axes `lead` are flattened"""
    rows = 1
    for size in lead:
        rows *= size
    return rows


def _check_stage(stage, M):
    torch = _torch()
    if tuple(stage.shape) != (M,) or stage.dtype != torch.int32 or not stage.is_contiguous():
        raise ValueError('stage must be a dense int32 tensor of shape ({0},), got {1} {2}'.format(M, stage.dtype, tuple(stage.shape)))


def _check_seg(seg):
    """nseg of the boundary table seg [nseg + 1]"""
    torch = _torch()
    if tuple(seg.shape) != (seg.numel(),) or seg.numel() < 1 or seg.dtype != torch.int32 or not seg.is_contiguous():
        raise ValueError('seg must be a dense int32 tensor of shape (nseg + 1,), got {0} {1}'.format(seg.dtype, tuple(seg.shape)))
    return int(seg.numel()) - 1


def _whiten(entry, X, taps, stage, q, skip, out, counts):
    """the checks of stage and X, the views, the check of out and the call that whiten_rows and whiten_rows_vector share; entry: the
    name in libshg, counts(rows): its two arguments in front of M"""
    torch = _torch()
    M, skip = int(X.shape[-1]), int(skip)
    lead = tuple(int(s) for s in X.shape[:-1])
    _check_stage(stage, M)
    if X.dtype != torch.float64:
        raise ValueError('X must be float64, got {0}'.format(X.dtype))
    front = counts(_row_count(lead))
    X, ldx = _rows_view(X, M)
    if out is None:
        out = torch.empty(lead + (max(M - skip, 0),), dtype=torch.float64, device=X.device)
    elif tuple(out.shape) != lead + (M - skip,) or out.dtype != torch.float64 or _rows_view(out, M - skip)[0] is not out:
        raise ValueError('out must be a float64 tensor of shape {0}, dense or a column slice of a matrix'.format(lead + (M - skip,)))
    _lib.call(entry, *front, M, _ptr(X), ldx, _ptr(stage), _ptr(taps), q, skip, _ptr(out), _rows_view(out, M - skip)[1], _stream())
    return out


def whiten_rows(X, taps, stage, channels=1, skip=0, out=None):
    """Decorrelation along the last axis of the device tensor X [..., M] (shg_whiten_rows): Y[..., t - skip] = sum_k h[n][k] X[..., t - k]
    for skip <= t < M with n = min(stage[t], q, t); the rows of X, all axes but the last flattened, belong to channel row % channels.
    taps [channels, q + 1, q + 1] (float64) and stage [M] (int32) are device tensors, as lstsq.whitening_taps and lstsq.arc_stages
    build them.  A two-dimensional X or out may be a column slice of a wider matrix (unit stride along the rows); anything else that
    is not dense is copied.  Returns out, or a new tensor [..., M - skip].
    Up to q = 128 the filter runs as a chain of FMAs per value (shg_whiten_rows); a longer one, q <= 4095, as a banded product on the
    fp64 MFMA (shg_whiten_rows_long), which needs the columns of X finite and repeats bitwise per call, not per tiling."""
    torch = require_gpu()
    channels = int(channels)
    if tuple(taps.shape) != (channels, taps.shape[-1], taps.shape[-1]) or taps.dtype != torch.float64 or not taps.is_contiguous():
        raise ValueError('taps must be a dense float64 tensor of shape ({0}, q + 1, q + 1), got {1}'.format(channels, tuple(taps.shape)))
    q = int(taps.shape[-1]) - 1
    return _whiten('shg_whiten_rows' if q <= WHITEN_ROWS_ORDER else 'shg_whiten_rows_long', X, taps, stage, q, skip, out,
                   lambda rows: (rows, channels))


def whiten_vector_info(dimension):
    """{'tile_columns'} of shg_whiten_rows_vector for models of that dimension: the output columns one workgroup takes.  Host only."""
    tile = ctypes.c_int(0)
    _lib.call('shg_whiten_vector_info', int(dimension), ctypes.byref(tile))
    return {'tile_columns': int(tile.value)}


def whiten_rows_vector(X, taps, stage, skip=0, out=None):
    """Decorrelation of vector noise along the last axis of the device tensor X [..., M] (shg_whiten_rows_vector): the rows of X, all
    axes but the last flattened, are groups of K consecutive rows, the K components of one series, and
    Y[g K + c, t - skip] = sum_k sum_c' H[n][k][c][c'] X[g K + c', t - k] for skip <= t < M with n = min(stage[t], q, t).  taps
    [q + 1, q + 1, K, K] (float64, 2 <= K <= 6, q <= 128) and stage [M] (int32) are device tensors, as lstsq.VectorNoise.taps and
    lstsq.arc_stages build them.  A two-dimensional X or out may be a column slice of a wider matrix (unit stride along the rows);
    anything else that is not dense is copied.  Returns out, or a new tensor [..., M - skip].  An output depends on the values of
    its group, stage[t] and the taps only, and repeats bitwise in every call and tiling."""
    torch = require_gpu()
    if taps.dim() != 4 or taps.shape[0] != taps.shape[1] or taps.shape[2] != taps.shape[3] or taps.dtype != torch.float64 or not taps.is_contiguous():
        raise ValueError('taps must be a dense float64 tensor of shape (q + 1, q + 1, K, K), got {0}'.format(tuple(taps.shape)))
    q, K = int(taps.shape[0]) - 1, int(taps.shape[2])

    def groups(rows):
        if K < 1 or rows % K:
            raise ValueError('the {0} rows of X are not groups of the {1} components of the model'.format(rows, K))
        return rows // K, K
    return _whiten('shg_whiten_rows_vector', X, taps, stage, q, skip, out, groups)


def segment_cross_lag_products(X, seg, lags, out=None):
    """Lagged products between the rows of the device tensor X [K, M], cut at arc boundaries (shg_segment_cross_lag_products):
    S[s, k, c, c'] = sum of X[c, t] X[c', t + k] over seg[s] <= t, t + k < seg[s + 1], for k = 0 .. lags (0 <= lags <= 128, 1 <= K <= 6):
    the empirical cross-covariance function of the components times the number of pairs.  seg [nseg + 1] (int32) holds the column
    indices of the boundaries, a device tensor; the kernel clamps it to 0 .. M and makes it non-decreasing.  X may be a column slice
    of a wider matrix (unit stride along the rows); anything else that is not dense is copied.  Returns out, or a new dense tensor
    [nseg, lags + 1, K, K]; every entry is written, and S[s, k, c, c] is bitwise segment_lag_products of row c."""
    torch = require_gpu()
    if X.dim() != 2 or X.dtype != torch.float64:
        raise ValueError('X must be a float64 tensor of shape (K, M), got {0} {1}'.format(X.dtype, tuple(X.shape)))
    K, M, lags = int(X.shape[0]), int(X.shape[1]), int(lags)
    nseg = _check_seg(seg)
    X, ldx = _rows_view(X, M)
    shape = (nseg, max(lags, 0) + 1, K, K)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=X.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError('out must be a dense float64 tensor of shape {0}'.format(shape))
    _lib.call('shg_segment_cross_lag_products', K, M, _ptr(X), ldx, lags, nseg, _ptr(seg), _ptr(out), _stream())
    return out


def segment_products(X, Bt, seg, channels=1, out=None):
    """Products of the rows of the device tensor X [..., M] with a basis, cut at arc boundaries (shg_segment_products):
    S[..., s, j] = sum of X[..., t] Bt[j, row % channels, t] over seg[s] <= t < seg[s + 1]; the rows of X, all axes but the last
    flattened, belong to channel row % channels.  Bt [u, channels, M] (float64, 1 <= u <= 16; [u, M] with channels = 1) is the basis,
    transformed like X and transposed, seg [nseg + 1] (int32) the column indices of the boundaries, both device tensors; the kernel
    clamps seg to 0 .. M and makes it non-decreasing.  A two-dimensional X may be a column slice of a wider matrix (unit stride along
    the rows), and so may Bt (the same stride for all its rows); anything else that is not dense is copied.  Returns out, or a new
    dense tensor [..., nseg, u]; every entry is written."""
    torch = require_gpu()
    M, channels = int(X.shape[-1]), int(channels)
    lead = tuple(int(s) for s in X.shape[:-1])
    if X.dtype != torch.float64:
        raise ValueError('X must be float64, got {0}'.format(X.dtype))
    if Bt.dim() == 2 and channels == 1:
        Bt = Bt.unsqueeze(1)
    if Bt.dim() != 3 or tuple(Bt.shape[1:]) != (channels, M) or Bt.dtype != torch.float64:
        raise ValueError('Bt must be a float64 tensor of shape (u, {0}, {1}), got {2}'.format(channels, M, tuple(Bt.shape)))
    u = int(Bt.shape[0])
    nseg = _check_seg(seg)
    X, ldx = _rows_view(X, M)
    ldb = int(Bt.stride(0) if channels == 1 else Bt.stride(1))              # rows j channels + c of Bt, one leading dimension
    if Bt.stride(2) != 1 or ldb < M or (channels > 1 and Bt.stride(0) != channels * ldb):
        Bt, ldb = Bt.contiguous(), M
    if out is None:
        out = torch.empty(lead + (nseg, u), dtype=torch.float64, device=X.device)
    elif tuple(out.shape) != lead + (nseg, u) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError('out must be a dense float64 tensor of shape {0}'.format(lead + (nseg, u)))
    _lib.call('shg_segment_products', _row_count(lead), channels, M, _ptr(X), ldx, _ptr(Bt), ldb, u, nseg, _ptr(seg), _ptr(out), _stream())
    return out


def _segment_lag_products(entry, X, seg, lags, out):
    """the views, checks and call that segment_lag_products and segment_lag_products_long share; entry: the name in libshg"""
    torch = require_gpu()
    M, lags = int(X.shape[-1]), int(lags)
    lead = tuple(int(s) for s in X.shape[:-1])
    if X.dtype != torch.float64:
        raise ValueError('X must be float64, got {0}'.format(X.dtype))
    nseg = _check_seg(seg)
    X, ldx = _rows_view(X, M)
    shape = lead + (nseg, max(lags, 0) + 1)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=X.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError('out must be a dense float64 tensor of shape {0}'.format(shape))
    _lib.call(entry, _row_count(lead), M, _ptr(X), ldx, lags, nseg, _ptr(seg), _ptr(out), _stream())
    return out


def segment_lag_products(X, seg, lags, out=None):
    """Lagged products of the rows of the device tensor X [..., M] with themselves, cut at arc boundaries (shg_segment_lag_products):
    S[..., s, k] = sum of X[..., t] X[..., t + k] over seg[s] <= t, t + k < seg[s + 1], for k = 0 .. lags (0 <= lags <= 128): lag 0 is
    the square sum of a segment, lags 0 .. q its empirical autocovariance times the number of pairs.  seg [nseg + 1] (int32) holds the
    column indices of the boundaries, a device tensor; the kernel clamps it to 0 .. M and makes it non-decreasing.  A two-dimensional
    X may be a column slice of a wider matrix (unit stride along the rows); anything else that is not dense is copied.  Returns out,
    or a new dense tensor [..., nseg, lags + 1]; every entry is written."""
    return _segment_lag_products('shg_segment_lag_products', X, seg, lags, out)


def segment_lag_products_long(X, seg, lags, out=None):
    """segment_lag_products for 0 <= lags <= 4095 on the fp64 MFMA (shg_segment_lag_products_long): the same arguments, views, checks
    and result, S[..., s, k] = sum of X[..., t] X[..., t + k] over seg[s] <= t, t + k < seg[s + 1].  Always the long kernel, whatever
    lags is; segment_lag_products never calls it.  An entry depends on the values of its segment and on k alone and repeats bitwise,
    but is not bitwise that of segment_lag_products (another summation order); the values inside a segment must be finite, columns
    outside every segment are not read.  segment_lag_long_info() gives the chunk length and the lags of an accumulator tile."""
    return _segment_lag_products('shg_segment_lag_products_long', X, seg, lags, out)


def segment_lag_long_info():
    """{'chunk', 'tile_lags', 'max_lags'} of shg_segment_lag_products_long: the columns of a work item, counted from the start of a
    segment, the lags of one accumulator tile and the largest lag.  Host only."""
    values = [ctypes.c_int(0) for _ in range(3)]
    _lib.call('shg_segment_lag_long_info', *(ctypes.byref(value) for value in values))
    return dict(zip(('chunk', 'tile_lags', 'max_lags'), (int(value.value) for value in values)))


WINDOW_SLOTS = 16                                                # slots of one shg_window_expand call: W <= E <= 16


def check_window_runs(run_slot, run_begin, n, W, E):
    """(run_slot, run_begin) of a shg_window_expand call as contiguous int32 arrays: run r covers the columns run_begin[r] ..
    run_begin[r + 1] - 1 of n and starts at slot run_slot[r].  ValueError unless 1 <= W <= E <= 16, run_begin ascends strictly from 0 to
    n and every run_slot lies in 0 .. E - W.  Host only."""
    n, W, E = int(n), int(W), int(E)
    if not 1 <= W <= E <= WINDOW_SLOTS:
        raise ValueError('a window of {0} fields in {1} slots: expected 1 <= W <= E <= {2}'.format(W, E, WINDOW_SLOTS))
    slot, begin = np.asarray(run_slot), np.asarray(run_begin)
    if slot.ndim != 1 or begin.shape != (slot.shape[0] + 1,) or slot.dtype.kind not in 'iu' or begin.dtype.kind not in 'iu':
        raise ValueError('run_slot [runs] and run_begin [runs + 1] must be integer arrays, got {0} and {1}'.format(slot.shape, begin.shape))
    if n < 0 or (n > 0 and slot.shape[0] < 1) or int(begin[0]) != 0 or int(begin[-1]) != n or np.any(np.diff(begin) <= 0):
        raise ValueError('run_begin must ascend strictly from 0 to the {0} columns'.format(n))
    if slot.size and (int(slot.min()) < 0 or int(slot.max()) > E - W):
        raise ValueError('a run starts at slot {0}, outside 0 .. E - W = {1}'.format(int(slot[(slot < 0) | (slot > E - W)][0]), E - W))
    return np.ascontiguousarray(slot, dtype=np.int32), np.ascontiguousarray(begin, dtype=np.int32)


def window_expand(T, factors, run_slot, run_begin, E, out=None):
    """The transposed design matrix of a block, expanded to the E slots of its time-variable parameters (shg_window_expand):
    S[e, ..., t] = factors[t, e - slot(t)] * T[..., t] inside the window slot(t) <= e < slot(t) + W of column t and +0.0 outside, with
    slot(t) = run_slot[r] along the columns run_begin[r] .. run_begin[r + 1] - 1 (host int tables, check_window_runs).  T [..., n] and
    factors [n, W] are float64 device tensors; a two-dimensional T may be a column slice of a wider matrix (unit stride along the
    rows), anything else that is not dense is copied.  Returns out, or a new dense tensor [E, ..., n]; every entry is written, the
    zeros included.  out [E, rows, n], if given, may be a view with strides (slot, row, 1) of a larger buffer: nothing else of it is
    touched."""
    torch = require_gpu()
    n, E = int(T.shape[-1]), int(E)
    lead = tuple(int(s) for s in T.shape[:-1])
    if T.dtype != torch.float64:
        raise ValueError('T must be float64, got {0}'.format(T.dtype))
    if factors.dim() != 2 or int(factors.shape[0]) != n or factors.dtype != torch.float64 or not factors.is_contiguous() or factors.device != T.device:
        raise ValueError('factors must be a dense float64 tensor of shape ({0}, W) beside T, got {1}'.format(n, tuple(factors.shape)))
    W = int(factors.shape[1])
    run_slot, run_begin = check_window_runs(run_slot, run_begin, n, W, E)
    if T.dim() == 2 and T.stride(1) == 1 and T.stride(0) >= n:
        ldt = int(T.stride(0))
    else:
        T, ldt = T.contiguous(), n
    rows = 1
    for size in lead:
        rows *= size
    if out is None:
        out = torch.empty((E,) + lead + (n,), dtype=torch.float64, device=T.device)
        lds, slot_stride = n, rows * n
    else:
        if tuple(out.shape) != (E, rows, n) or out.dtype != torch.float64 or out.device != T.device or (n > 1 and out.stride(2) != 1):
            raise ValueError('out must be a float64 tensor of shape ({0}, {1}, {2}) with unit stride along the columns'.format(E, rows, n))
        lds = int(out.stride(1)) if rows > 1 else max(int(out.stride(1)), n)
        slot_stride = int(out.stride(0)) if E > 1 else max(int(out.stride(0)), (rows - 1) * lds + n)
        if lds < n or slot_stride < (rows - 1) * lds + n:
            raise ValueError('the rows or the slots of out overlap (strides {0})'.format(tuple(out.stride())))
        Plan._written(out)
    _lib.call('shg_window_expand', rows, n, _ptr(T), ldt, _host_ptr(run_slot), _host_ptr(run_begin), int(run_slot.shape[0]), _ptr(factors), W, E,
              _ptr(out), lds, slot_stride, _stream())
    return out


class OrderMajorSeries:
    """A time series of coefficient sets that stays on the device between operators (the batching of TimeSeries.to_array,
    grates/gravityfield.py:964-980, in the layout the order-wise operators work on): `data` [(N+1)^2, Bpad] with the epochs fastest
    (Bpad = epochs rounded up to 32) and the coefficients of one order and kind (the slots of the DDK block list: order 0 cosine,
    order 1 cosine, order 1 sine, ...) in consecutive rows.  `OrderWiseFilter.filter_series` and `Plan.synthesis` take and return it
    without passing through the reference arrays [B, N+1, N+1]; `from_batch` / `to_batch` convert."""

    def __init__(self, data, max_degree, epochs):
        self.data, self.max_degree, self.epochs = data, int(max_degree), int(epochs)

    @property
    def padded_epochs(self):
        return int(self.data.shape[1])

    @classmethod
    def from_batch(cls, anm):
        torch = require_gpu()
        x = to_device(anm)
        if x.dim() != 3 or x.shape[1] != x.shape[2]:
            raise ValueError('coefficient batch must have shape (B, N+1, N+1), got {0}'.format(tuple(x.shape)))
        B, N = int(x.shape[0]), int(x.shape[1]) - 1
        bpad = -(-max(B, 1) // 32) * 32
        data = torch.empty(((N + 1) ** 2, bpad), dtype=torch.float64, device=x.device)
        _lib.call('shg_order_major_pack', _ptr(x), N, B, _ptr(data), bpad, _stream())
        return cls(data, N, B)

    def to_batch(self):
        torch = require_gpu()
        N, B = self.max_degree, self.epochs
        out = torch.empty((B, N + 1, N + 1), dtype=torch.float64, device=self.data.device)
        _lib.call('shg_order_major_unpack', _ptr(self.data), N, B, self.padded_epochs, _ptr(out), _stream())
        return out

    @property
    def values(self):
        """the coefficients of the epochs that exist, [(N+1)^2, B]: a view of `data` (row stride = padded epochs)"""
        return self.data[:, :self.epochs]

    def like(self, data):
        return OrderMajorSeries(data, self.max_degree, self.epochs)

    def truncated(self, max_degree):
        """the series of the degrees up to `max_degree` (<= the own one): rows gathered on the device"""
        if max_degree == self.max_degree:
            return self
        if max_degree > self.max_degree:
            raise ValueError('the series holds degrees up to {0}'.format(self.max_degree))
        torch = require_gpu()
        N, M = self.max_degree, int(max_degree)
        rows = np.concatenate([order_major_first_row(N, s) + np.arange(M + 1 - ((s + 1) >> 1)) for s in range(2 * M + 1)])
        index = torch.from_numpy(rows.astype(np.int64)).to(self.data.device)
        return OrderMajorSeries(self.data.index_select(0, index), M, self.epochs)

    def to_array(self, min_degree=0):
        """[B, P] device tensor of the degree-wise vectors (TimeSeries.to_array, grates/gravityfield.py:973-980)"""
        torch = require_gpu()
        index = torch.from_numpy(order_major_rows_of_degreewise(self.max_degree, min_degree)).to(self.data.device)
        return self.values.index_select(0, index).t().contiguous()


def order_major_first_row(N, s):
    """first row of slot s (0: order 0 cosine, 2m - 1: order m cosine, 2m: order m sine) in a series of degree N (csrc/filters.hip: om_row)"""
    if s == 0:
        return 0
    m = (s + 1) >> 1
    cos_row = (N + 1) + 2 * ((m - 1) * (N + 1) - m * (m - 1) // 2)
    return cos_row if s & 1 else cos_row + (N + 1 - m)


_om_index_cache = {}


def order_major_rows_of_degreewise(N, min_degree=0):
    """int64 [P]: the row of an order-major series of degree N that holds entry p of the degree-wise vector of the degrees min_degree .. N
    (the order of utilities.ravel_coefficients: C_n0, C_n1, S_n1, C_n2, ... per degree)"""
    key = (int(N), int(min_degree))
    if key not in _om_index_cache:
        rows = []
        for n in range(min_degree, N + 1):
            rows.append(order_major_first_row(N, 0) + n)
            for m in range(1, n + 1):
                rows.append(order_major_first_row(N, 2 * m - 1) + n - m)
                rows.append(order_major_first_row(N, 2 * m) + n - m)
        _om_index_cache[key] = np.asarray(rows, dtype=np.int64)
    return _om_index_cache[key]


def degree_scale_series(series, weights, first_degree=0):
    """degree-wise scaling (Gaussian / Butterworth) of every epoch of an OrderMajorSeries; degrees below `first_degree` are copied"""
    torch = require_gpu()
    w = to_device(weights)
    if w.numel() != series.max_degree + 1:
        raise ValueError('weights must have max_degree + 1 entries')
    out = torch.empty_like(series.data)
    _lib.call('shg_degree_scale_om', _ptr(w), series.max_degree, int(first_degree), _ptr(series.data), series.epochs, series.padded_epochs, _ptr(out), _stream())
    return series.like(out)


def orderwise_filter_series(blocks_packed, block_offsets, block_max_degree, series):
    """OrderWiseFilter.filter of every epoch of an OrderMajorSeries: one matrix product per block, nothing gathered or scattered."""
    torch = require_gpu()
    out = torch.empty_like(series.data)
    _lib.call('shg_orderwise_filter_om', _ptr(blocks_packed), _ptr(block_offsets), int(block_max_degree), series.max_degree,
              _ptr(series.data), series.epochs, series.padded_epochs, _ptr(out), _stream())
    return OrderMajorSeries(out, series.max_degree, series.epochs)


def orderwise_filter(blocks_packed, block_offsets, block_max_degree, anm):
    """blocks_packed: 1d device tensor, block_offsets: int64 device tensor [2Nb+1]; anm [B, N+1, N+1]."""
    torch = require_gpu()
    x = to_device(anm)
    out = torch.empty_like(x)
    _lib.call('shg_orderwise_filter', _ptr(blocks_packed), _ptr(block_offsets), int(block_max_degree), x.shape[-1] - 1,
              _ptr(x), x.shape[0], _ptr(out), _stream())
    return out


def orderwise_filter_info(N, B):
    """{'via_series', 'group', 'lds_bytes', 'epochs_per_workgroup'}: the kernels `orderwise_filter` takes for B epochs of degree N -- whether the
    batch goes through the order-major layout, and the orders per workgroup (8, 4, 2; 0: refused) and LDS bytes of the kernel on the reference
    layout.  A host-side query: no GPU needed."""
    arr = (ctypes.c_int * 4)()
    _lib.call('shg_orderwise_filter_info', int(N), int(B), arr)
    return {'via_series': bool(arr[0]), 'group': int(arr[1]), 'lds_bytes': int(arr[2]), 'epochs_per_workgroup': int(arr[3])}


def ddk_blocks(normal_blocks, weights):
    """W_k = (N_k + diag(w[m:]))^-1 N_k for a list of order-wise normal blocks (host ndarrays) -> list of ndarrays."""
    torch = require_gpu()
    nb = normal_blocks[0].shape[0] - 1
    sizes = np.array([b.size for b in normal_blocks], dtype=np.int64)
    offsets = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    packed = to_device(np.concatenate([np.ascontiguousarray(b, dtype=np.float64).ravel() for b in normal_blocks]))
    off = torch.from_numpy(offsets).to(packed.device)
    work, out = torch.empty_like(packed), torch.empty_like(packed)
    w = to_device(weights)
    _lib.call('shg_ddk_blocks', _ptr(packed), _ptr(off), int(nb), _ptr(w), _ptr(work), _ptr(out), _stream())
    host = to_host(out)
    return [host[o:o + s].reshape(b.shape).copy() for o, s, b in zip(offsets, sizes, normal_blocks)]


def dense_filter(W, X):
    """Y = W @ X, W [P, P], X [P, T] device tensors."""
    torch = require_gpu()
    W, X = to_device(W), to_device(X)
    out = torch.empty_like(X)
    _lib.call('shg_dense_filter', _ptr(W), W.shape[0], _ptr(X), X.shape[1], _ptr(out), _stream())
    return out


def spd_solve(A, B):
    """X = A^-1 B for symmetric positive definite A (device Cholesky)."""
    torch = require_gpu()
    A, B = to_device(A), to_device(B)
    out = torch.empty_like(B)
    _lib.call('shg_spd_solve', _ptr(A), A.shape[0], _ptr(B), B.shape[1], _ptr(out), _stream())
    return out


def dgemm(A, B):
    """C = A @ B on the fp64 MFMA GEMM (row-major device tensors)."""
    torch = require_gpu()
    A, B = to_device(A), to_device(B)
    M, K = A.shape
    N = B.shape[1]
    out = torch.empty((M, N), dtype=torch.float64, device=A.device)
    _lib.call('shg_dgemm', M, N, K, _ptr(A), K, _ptr(B), N, _ptr(out), N, _stream())
    return out


def gemm(A, B, transa=False, transb=False, alpha=1.0, beta=0.0, out=None):
    """out = alpha op(A) op(B) + beta out on the fp64 MFMA GEMM; A, B, out are 2-d row-major device tensors
    (row strides are honoured, the last dimension must be contiguous)."""
    torch = require_gpu()
    A = A if isinstance(A, torch.Tensor) and A.is_cuda and A.dtype == torch.float64 else to_device(A)
    B = B if isinstance(B, torch.Tensor) and B.is_cuda and B.dtype == torch.float64 else to_device(B)
    for t in (A, B):
        if t.dim() != 2 or (t.numel() > 0 and t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError('gemm operands must be two-dimensional with a contiguous last dimension')
    M = A.shape[1] if transa else A.shape[0]
    K = A.shape[0] if transa else A.shape[1]
    Kb = B.shape[1] if transb else B.shape[0]
    N = B.shape[0] if transb else B.shape[1]
    if K != Kb:
        raise ValueError('gemm: inner dimensions differ ({0} vs {1})'.format(K, Kb))
    if out is None:
        if beta != 0.0:
            raise ValueError('gemm: beta != 0 needs an output tensor')
        out = torch.empty((M, N), dtype=torch.float64, device=A.device)
    elif tuple(out.shape) == (M, N) and not (N > 1 and out.stride(1) != 1):
        Plan._written(out)
    if tuple(out.shape) != (M, N) or (N > 1 and out.stride(1) != 1):
        raise ValueError('gemm: output must be ({0}, {1}) with a contiguous last dimension'.format(M, N))
    _lib.call('shg_gemm', int(transa), int(transb), M, N, K, float(alpha), _ptr(A), max(A.stride(0), 1), _ptr(B), max(B.stride(0), 1),
              float(beta), _ptr(out), max(out.stride(0), 1), _stream())
    return out


# flags of shg_gemm_ex (include/shg.h): triangular operands and the upper-tiles-only launch
GEMM_A_UPPER, GEMM_A_LOWER, GEMM_B_UPPER, GEMM_B_LOWER, GEMM_UPPER_ONLY = 1, 2, 4, 8, 16
GEMM_ROUTE_KINDS = ('NONE', 'TALL', 'GEMV', 'PANEL', 'TILE64', 'TILE128', 'SCALE')      # shg_gemm_route_kind


def _address(x):
    return int(x) if isinstance(x, int) else int(x.data_ptr())


def gemm_route(transa, transb, M, N, K, A, lda, strideA, B, ldb, strideB, C, ldc, strideC, batch=1, flags=0):
    """The kernels shg_gemm_ex (and shg_gemm: strides 0, batch 1, flags 0) would launch for these arguments, as a dict.
    A, B, C are tensors or plain addresses (alignment and aliasing steer the choice; nothing is read).  Host logic only:
    works without a GPU.  Raises ShgError for arguments that shg_gemm_ex refuses."""
    which = (ctypes.c_int64 * 8)()
    _lib.call('shg_gemm_route', int(bool(transa)), int(bool(transb)), M, N, K, 1.0, ctypes.c_void_p(_address(A)), lda, strideA,
              ctypes.c_void_p(_address(B)), ldb, strideB, 0.0, ctypes.c_void_p(_address(C)), ldc, strideC, batch, flags, which)
    route = {'kind': GEMM_ROUTE_KINDS[which[0]], 'slices': which[1], 'chunk': which[2], 'strips': bool(which[3]), 'm_main': which[4],
             'a_lower': bool(which[5] & 1), 'b_upper': bool(which[5] & 2), 'alias': {0: '', 1: 'A', 2: 'B', 3: 'AB'}[which[6]], 'rest': None}
    if which[4] > 0:
        route['rest'] = {'kind': GEMM_ROUTE_KINDS[which[7] & 255], 'slices': (which[7] >> 8) & 255, 'strips': bool(which[7] >> 16 & 1)}
    return route


COVPROP_ROUTE_KINDS = ('NONE', 'ROWS', 'DIRECT', 'REGISTER', 'PADDED', 'SYMMETRIC')      # shg_covprop_route_kind


def covprop_route(nlon, P, aligned, M, symmetric):
    """The kernel Plan.covariance_propagation(method='direct') runs for a band of M grid rows on nlon meridians and a P x P matrix
    whose base address is (aligned) or is not a multiple of 16 bytes: one of COVPROP_ROUTE_KINDS.  Host logic only: works without a GPU."""
    lib = _lib.load()
    kind = lib.shg_covprop_route(int(nlon), int(P), int(bool(aligned)), int(M), int(bool(symmetric)))
    if kind < 0:
        raise _lib.ShgError('shg_covprop_route', kind, lib.shg_last_error().decode())
    return COVPROP_ROUTE_KINDS[kind]


def gemm_ex_args(A, B, out, transa=False, transb=False):
    """(transa, transb, M, N, K, A, lda, strideA, B, ldb, strideB, out, ldc, strideC, batch) of a call of gemm_ex -- the leading
    arguments of gemm_route.  Operands are 2-d, or 3-d [batch][rows][columns]; a 2-d operand beside 3-d ones is repeated (stride 0)."""
    batch = 1
    for t in (A, B, out):
        if t.dim() not in (2, 3) or (t.numel() > 0 and t.shape[-1] > 1 and t.stride(-1) != 1):
            raise ValueError('gemm_ex operands must be two- or three-dimensional with a contiguous last dimension')
        if t.dim() == 3:
            if batch != 1 and t.shape[0] != batch:
                raise ValueError('gemm_ex: batch counts differ')
            batch = t.shape[0]
    if out.dim() == 2 and batch != 1:
        raise ValueError('gemm_ex: a batch needs a three-dimensional output')
    M = A.shape[-1] if transa else A.shape[-2]
    K = A.shape[-2] if transa else A.shape[-1]
    Kb = B.shape[-1] if transb else B.shape[-2]
    N = B.shape[-2] if transb else B.shape[-1]
    if K != Kb:
        raise ValueError('gemm_ex: inner dimensions differ ({0} vs {1})'.format(K, Kb))
    if tuple(out.shape[-2:]) != (M, N):
        raise ValueError('gemm_ex: output must be ({0}, {1})'.format(M, N))
    stride = lambda t: t.stride(0) if t.dim() == 3 and t.shape[0] > 1 else 0      # noqa: E731
    # a single row is never stepped over: torch leaves the stride of an axis of size 1 arbitrary (1 for the transpose of a column)
    ld = lambda t: max(t.stride(-2), 1) if t.shape[-2] > 1 else max(t.stride(-2), t.shape[-1], 1)      # noqa: E731
    return (bool(transa), bool(transb), M, N, K, A, ld(A), stride(A), B, ld(B), stride(B), out, ld(out), stride(out), batch)


def gemm_ex(A, B, out, transa=False, transb=False, alpha=1.0, beta=0.0, flags=0):
    """out_i = alpha op(A_i) op(B_i) + beta out_i on the fp64 MFMA GEMM for device tensors (see gemm_ex_args): strided batches,
    triangular operands (GEMM_A_UPPER ...: the zero side is not read) and GEMM_UPPER_ONLY (output tiles entirely below the
    diagonal are not written).  shg_gemm_ex of include/shg.h; `out` may be B or A in the in-place forms listed there."""
    torch = require_gpu()
    for t in (A, B, out):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64):
            raise ValueError('gemm_ex: fp64 device tensors expected')
    ta, tb, M, N, K, A, lda, sA, B, ldb, sB, out, ldc, sC, batch = gemm_ex_args(A, B, out, transa, transb)
    Plan._written(out)
    _lib.call('shg_gemm_ex', int(ta), int(tb), M, N, K, float(alpha), _ptr(A), lda, sA, _ptr(B), ldb, sB, float(beta), _ptr(out), ldc, sC, batch,
              int(flags), _stream())
    return out


def potrf(A, check=True):
    """Upper Cholesky factor U (A = U^T U) of a symmetric positive definite device matrix, in place; the strictly lower
    triangle is zeroed.  Raises numpy.linalg.LinAlgError like scipy.linalg.cholesky when a pivot is not positive."""
    torch = require_gpu()
    if A.dim() != 2 or A.shape[0] != A.shape[1] or (A.shape[1] > 1 and A.stride(1) != 1):
        raise ValueError('potrf: square matrix with a contiguous last dimension expected')
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    _lib.call('shg_potrf', A.shape[0], _ptr(A), max(A.stride(0), 1), _ptr(info), _stream())
    if check:
        k = int(info.item())
        if k:
            import numpy as np
            raise np.linalg.LinAlgError('{0}-th leading minor of the array is not positive definite'.format(k))
    return A


def trtri(U):
    """Inverse of an upper triangular device matrix (new tensor)."""
    torch = require_gpu()
    if U.dim() != 2 or U.shape[0] != U.shape[1] or (U.shape[1] > 1 and U.stride(1) != 1):
        raise ValueError('trtri: square matrix with a contiguous last dimension expected')
    X = torch.empty((U.shape[0], U.shape[0]), dtype=torch.float64, device=U.device)
    _lib.call('shg_trtri', U.shape[0], _ptr(U), max(U.stride(0), 1), _ptr(X), max(X.stride(0), 1), _stream())
    return X


def transpose_in_place(A):
    """A <- A^T for a square 2-d device tensor with a contiguous last dimension, in its own storage"""
    require_gpu()
    if A.dim() != 2 or A.shape[0] != A.shape[1] or (A.shape[1] > 1 and A.stride(1) != 1):
        raise ValueError('transpose_in_place: a square matrix with a contiguous last dimension is expected')
    _lib.call('shg_transpose_in_place', A.shape[0], _ptr(A), max(A.stride(0), 1), _stream())
    return A


def axpby(alpha, X, beta, Y):
    """Y = alpha X + beta Y in place for 2-d device tensors of equal shape (row strides honoured)."""
    require_gpu()
    if X.dim() != 2 or tuple(X.shape) != tuple(Y.shape):
        raise ValueError('axpby: two-dimensional operands of equal shape expected')
    if X.numel() == 0:
        return Y
    if (X.shape[1] > 1 and X.stride(1) != 1) or (Y.shape[1] > 1 and Y.stride(1) != 1):
        raise ValueError('axpby: contiguous last dimension expected')
    Plan._written(Y)
    _lib.call('shg_axpby', X.shape[0], X.shape[1], float(alpha), _ptr(X), max(X.stride(0), 1), float(beta), _ptr(Y), max(Y.stride(0), 1), _stream())
    return Y


JACOBI_MAX = 128       # the largest r and c of shg_jacobi_svd: one matrix must fit the LDS of a CU
_UNIT_ROUNDOFF = 2.0 ** -53


def _jacobi(G, max_sweeps, name):
    """shg_jacobi_svd in place on a contiguous fp64 device tensor [batch, r, c] -> (V [batch, c, c], sigma [batch, c], sweeps [batch]
    int32), raising numpy.linalg.LinAlgError when a matrix needed more than max_sweeps sweeps"""
    torch = require_gpu()
    batch, r, c = (int(s) for s in G.shape)
    V = torch.empty((batch, c, c), dtype=torch.float64, device=G.device)
    sigma = torch.empty((batch, c), dtype=torch.float64, device=G.device)
    sweeps = torch.empty((batch,), dtype=torch.int32, device=G.device)
    _lib.call('shg_jacobi_svd', _ptr(G), c, r * c, _ptr(V), c, c * c, _ptr(sigma), r, c, batch, int(max_sweeps), _ptr(sweeps), _stream())
    if int(sweeps.min().item()) < 0:
        raise np.linalg.LinAlgError('{0}: the Jacobi rotations did not converge within {1} sweeps'.format(name, int(max_sweeps)))
    return V, sigma, sweeps


def _small_matrices(X, name, square):
    """(copy [batch, r, c] of the fp64 device tensor X [r, c] or [batch, r, c], whether X was a batch) for the LDS kernels"""
    torch = require_gpu()
    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float64 and X.dim() in (2, 3)):
        raise ValueError('{0}: a float64 device tensor [r, c] or [batch, r, c] is expected'.format(name))
    r, c = int(X.shape[-2]), int(X.shape[-1])
    if square and r != c:
        raise ValueError('{0}: square matrices expected, got {1} x {2}'.format(name, r, c))
    if not (1 <= c <= r <= JACOBI_MAX) or (X.dim() == 3 and X.shape[0] < 1):
        raise ValueError('{0}: {1} x {2} is outside 1 <= columns <= rows <= {3}'.format(name, r, c, JACOBI_MAX))
    return X.reshape(-1, r, c).clone(memory_format=torch.contiguous_format), X.dim() == 3


def jacobi_svd(G, max_sweeps=30):
    """(U, s, Vt, sweeps) with G = U diag(s) Vt for a float64 device tensor G [r, c] or [batch, r, c], c <= r <= 128, by one-sided Jacobi
    rotations in LDS (shg_jacobi_svd, one workgroup per matrix; G is not changed).  s descends; U [.., r, c] is the rotated G over s,
    with zero columns where s == 0; Vt [.., c, c] is orthogonal.  sweeps: the sweeps the kernel used (an int, or an int32 tensor
    [batch]).  The order of the rotations is fixed: repeated calls are bitwise equal.  Raises numpy.linalg.LinAlgError when a matrix
    has not converged after max_sweeps sweeps."""
    torch = require_gpu()
    work, batched = _small_matrices(G, 'jacobi_svd', False)
    V, sigma, sweeps = _jacobi(work, max_sweeps, 'jacobi_svd')
    s, order = torch.sort(sigma, dim=1, descending=True, stable=True)
    pick = order.unsqueeze(1)
    GV = torch.gather(work, 2, pick.expand(-1, work.shape[1], -1))
    scale = torch.where(s > 0.0, s, torch.ones_like(s)).unsqueeze(1)
    U = torch.where((s > 0.0).unsqueeze(1), GV / scale, torch.zeros_like(GV))
    Vt = torch.gather(V, 2, pick.expand(-1, V.shape[1], -1)).transpose(1, 2).contiguous()
    if batched:
        return U, s, Vt, sweeps
    return U[0], s[0], Vt[0], int(sweeps.item())


def syev(A, max_sweeps=30):
    """(w, v, sweeps): eigenvalues w ascending and eigenvectors v (columns) of the symmetric float64 device tensor A [n, n] or
    [batch, n, n], n <= 128, of which only the upper triangle is read, by shg_jacobi_svd.  One-sided Jacobi diagonalises A^T A = A^2,
    which cannot tell lambda from -lambda, so the kernel works on A + sigma0 I with the Gershgorin shift
    sigma0 = max(0, max_i(sum_{j != i} |a_ij| - a_ii)), which is positive semi-definite: its right singular vectors are the
    eigenvectors of A, and w_i = v_i . (A + sigma0 I) v_i - sigma0 (the Rayleigh quotients; the second factor is the kernel's rotated
    matrix).  sweeps as in jacobi_svd; numpy.linalg.LinAlgError when max_sweeps did not suffice."""
    torch = require_gpu()
    work, batched = _small_matrices(A, 'syev', True)
    work = torch.triu(work)
    work = work + torch.triu(work, 1).transpose(1, 2)
    diagonal = torch.diagonal(work, dim1=1, dim2=2)
    shift = (work.abs().sum(dim=2) - diagonal.abs() - diagonal).amax(dim=1).clamp_min(0.0)
    diagonal += shift.unsqueeze(1)              # a view: the diagonal of work
    V, _, sweeps = _jacobi(work, max_sweeps, 'syev')
    w = (V * work).sum(dim=1) - shift.unsqueeze(1)
    w, order = torch.sort(w, dim=1, stable=True)
    v = torch.gather(V, 2, order.unsqueeze(1).expand(-1, V.shape[1], -1))
    if batched:
        return w, v, sweeps
    return w[0], v[0], int(sweeps.item())


def orthonormalise(B):
    """Q [m, k] with orthonormal columns that span those of the tall float64 device tensor B [m, k], k <= 128, m >= k, by shifted
    CholeskyQR3 (Fukaya, Kannan, Nakatsukasa, Yamamoto, Yanagisawa, SIAM J. Sci. Comput. 42, 2020) on the fp64 MFMA: the Gram matrix
    B^T B + s I with s = 11 (m k + k (k + 1)) u |B|_F^2, its Cholesky factor R (potrf), Q = B R^-1 (trtri, gemm), then two plain
    CholeskyQR passes.  The shift bounds cond(Q) of the first pass by about u^-1/2 for cond(B) up to about 1 / (u sqrt(11 m k)).
    Raises numpy.linalg.LinAlgError when B is numerically rank deficient: a pivot of the second or third pass that is not positive,
    or a pivot of the second pass at or below u -- a column whose part outside the span of the earlier ones is smaller than the
    shift, which the second pass would otherwise scale up from rounding noise to a unit vector."""
    torch = require_gpu()
    if not (isinstance(B, torch.Tensor) and B.is_cuda and B.dtype == torch.float64 and B.dim() == 2):
        raise ValueError('orthonormalise: a two-dimensional float64 device tensor is expected')
    m, k = int(B.shape[0]), int(B.shape[1])
    if not (1 <= k <= JACOBI_MAX and m >= k):
        raise ValueError('orthonormalise: {0} x {1} is outside 1 <= columns <= {2}, rows >= columns'.format(m, k, JACOBI_MAX))
    Q = B
    for step in range(3):
        gram = gemm(Q, Q, transa=True)
        if step == 0:
            shift = 11.0 * (m * k + k * (k + 1)) * _UNIT_ROUNDOFF * float(torch.diagonal(gram).sum().item())
            torch.diagonal(gram).add_(shift)
        try:
            potrf(gram)
        except np.linalg.LinAlgError as err:
            if step == 0:
                raise np.linalg.LinAlgError('orthonormalise: the shifted Gram matrix is not positive definite (non-finite input?)') from err
            raise np.linalg.LinAlgError('orthonormalise: the columns are numerically rank deficient (pass {0}: {1})'.format(step + 1, err)) from err
        if step == 1 and not float(torch.diagonal(gram).min().item()) ** 2 > _UNIT_ROUNDOFF:
            raise np.linalg.LinAlgError('orthonormalise: the columns are numerically rank deficient (a pivot of pass 2 is at rounding level)')
        Q = gemm(Q, trtri(gram))
    return Q
