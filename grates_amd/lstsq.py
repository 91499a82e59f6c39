"""
Block-banded normal equations on the device: the reference's vector-autoregressive constraint models, sparse
`BlockMatrix` and `NormalEquations` ("Kalman smoother", grates/lstsq.py:12-1149) with the same class and method
names, argument meaning and error behaviour.  The host keeps the reference's loops over non-zero blocks; every block
lives in HBM as its own fp64 tensor and every block operation is a libshg call:

    block products                  -> shg_gemm  (fp64 MFMA, transposes / alpha / beta, accumulates in place)
    scipy.linalg.cholesky           -> shg_potrf (blocked right-looking upper Cholesky)
    solve_triangular / inv of a
    diagonal factor block           -> shg_trtri once per diagonal block (cached), then shg_gemm
    block scaling / accumulation    -> shg_axpby

Vectors may be passed as NumPy arrays (results come back as NumPy arrays, like the reference) or as device tensors
(results stay on the device).  There is no CPU fallback.

Dense eigen and singular value decompositions (teigh, trsvd, and UnscentedTransformSymmetric on their results) run on
shg_jacobi_svd, one-sided Jacobi rotations in LDS, with the products around it on shg_gemm.

Not built: AutoregressiveModel.from_transformed_coefficients (pseudo-inverse).
"""

import collections
import weakref

import numpy as np

from . import engine


def _is_tensor(x):
    return engine._torch().is_tensor(x)


def _dev(x):
    """fp64 device tensor (copy) of an ndarray / tensor"""
    torch = engine.require_gpu()
    if torch.is_tensor(x):
        return x.to(device=engine.device(), dtype=torch.float64).clone(memory_format=torch.contiguous_format)   # dense row-major, whatever the strides of x
    return engine.to_device(np.asarray(x, dtype=np.float64))


def _zeros(shape):
    torch = engine.require_gpu()
    return torch.zeros(tuple(int(s) for s in shape), dtype=torch.float64, device=engine.device())


def _dot(a, b):
    """sum of the element-wise product of two [n, k] device tensors (trace of a^T b on the MFMA GEMM)"""
    return float(np.trace(engine.to_host(engine.gemm(a, b, transa=True))))


def _like_input(result, template):
    return result if _is_tensor(template) else engine.to_host(result)


class AutoregressiveModel:
    """VAR(p) model x_t = sum_k B_k x_(t-k) + w_t given by its coefficient matrices B_1 .. B_p and the covariance matrix of
    the white noise w (grates/lstsq.py:12-247)."""

    def __init__(self, coefficients, covariance_matrix):
        # an ndarray of stacked matrices is split along its first axis (upstream behaviour); lists / tuples are kept as given
        self.__coefficients = tuple(coefficients) if isinstance(coefficients, np.ndarray) else coefficients
        self.__covariance_matrix = covariance_matrix
        self.__normal_equation = None           # BlockMatrix of the pseudo-observation normals, built on first use

    @property
    def dimension(self):
        return self.__covariance_matrix.shape[0]

    @property
    def order(self):
        return len(self.__coefficients)

    @property
    def white_noise_covariance(self):
        return self.__covariance_matrix

    @property
    def coefficients(self):
        return self.__coefficients

    def order_one_representation(self):
        """grates/lstsq.py:81-99"""
        if self.order == 1:
            return self
        B = np.eye(self.dimension * self.order)
        for k in range(self.order):
            B[0:self.dimension, k * self.dimension:(k + 1) * self.dimension] = np.asarray(self.__coefficients[k]).copy()
        Q = np.zeros(B.shape)
        Q[0:self.dimension, 0:self.dimension] = np.asarray(self.__covariance_matrix).copy()
        return AutoregressiveModel(B, Q)

    @staticmethod
    def from_covariance_function(covariance_function):
        """Yule-Walker equations solved with the block Cholesky factorisation on the device (grates/lstsq.py:127-167)."""
        lags = tuple(covariance_function)                      # Sigma_0 .. Sigma_p (an ndarray is split along its first axis)
        p = len(lags) - 1
        if p == 0:
            return AutoregressiveModel((), lags[0])
        d = lags[0].shape[0]
        bounds = list(range(0, (p + 1) * d, d))               # p blocks of size d
        # block Toeplitz system of the Yule-Walker equations, upper blocks only: T[r, c] = Sigma_(c - r)^T, rhs rows = Sigma_(r + 1)
        coefficient_matrix = BlockMatrix(bounds, bounds)
        for r in range(p):
            for c in range(r, p):
                coefficient_matrix[r, c] = np.ascontiguousarray(lags[c - r].T)
        right_hand_side = np.vstack([lags[r + 1] for r in range(p)])
        covariance_function = lags
        model_order = p

        coefficient_matrix.cholesky()
        rhs = _dev(right_hand_side)
        x1 = coefficient_matrix.solve_triangular(rhs, transpose=True)
        x2 = coefficient_matrix.solve_triangular(x1)
        Q = _dev(covariance_function[0])
        engine.gemm(x2, rhs, transa=True, alpha=-1.0, beta=1.0, out=Q)
        return AutoregressiveModel(np.split(engine.to_host(x2).T, model_order, axis=1), engine.to_host(Q))

    @staticmethod
    def from_sample(sample, order):
        """grates/lstsq.py:170-190 (as upstream: every lag uses the zero-lag product)"""
        s = _dev(sample)
        product = engine.to_host(engine.gemm(s, s, transa=True))
        covariance_function = [product / (sample.shape[0] - k) for k in range(order + 1)]
        return AutoregressiveModel.from_covariance_function(covariance_function)

    def __compute_normals(self):
        """Normal equations of the pseudo-observations of the model (grates/lstsq.py:192-209): W = chol(Q) (upper),
        observation blocks W^-T B_k (k descending) and -W^-T, normal blocks as their products."""
        W = engine.potrf(_dev(self.__covariance_matrix))
        Winv = engine.trtri(W)
        observation_equations = [engine.gemm(Winv, _dev(B), transa=True) for B in self.__coefficients[::-1]]
        minus = _zeros(Winv.shape)
        engine.axpby(-1.0, Winv.t().contiguous(), 0.0, minus)
        observation_equations.append(minus)

        count = self.order + 1
        bounds = list(range(0, (count + 1) * self.dimension, self.dimension))
        self.__normal_equation = BlockMatrix(bounds, bounds)
        for r, left in enumerate(observation_equations):
            for c in range(r, count):
                self.__normal_equation._set_device(r, c, engine.gemm(left, observation_equations[c], transa=True))

    def normal_equation_block(self, row, column):
        """normal-equation block (row, column) as ndarray (grates/lstsq.py:211-230)"""
        return engine.to_host(self._normal_equation_block_device(row, column))

    def _normal_equation_block_device(self, row, column):
        if self.__normal_equation is None:
            self.__compute_normals()
        return self.__normal_equation.device_block(row, column)

    def to_transformed_coefficients(self):
        """grates/lstsq.py:232-247"""
        W_inv = engine.trtri(engine.potrf(_dev(self.__covariance_matrix)))
        transformed = [engine.to_host(engine.gemm(W_inv, _dev(B), alpha=-1.0)) for B in self.__coefficients[::-1]]
        transformed.append(engine.to_host(W_inv))
        return np.hstack(transformed)


class AutoregressiveModelSequence:
    """Sequence of VAR models of increasing order, starting from order 0 (grates/lstsq.py:250-411)."""

    def __init__(self, armodels):
        self.__armodels = armodels

    @staticmethod
    def from_covariance_function(covariance_function):
        return AutoregressiveModelSequence([AutoregressiveModel.from_covariance_function(covariance_function[0:k + 1])
                                            for k in range(len(covariance_function))])

    @staticmethod
    def from_sample(sample, maximum_order):
        return AutoregressiveModelSequence([AutoregressiveModel.from_sample(sample, order) for order in range(maximum_order + 1)])

    @property
    def models(self):
        """the AR models of orders 0 .. maximum_order, as given (no reference counterpart: whitening_taps reads them)"""
        return tuple(self.__armodels)

    @property
    def maximum_order(self):
        return self.__armodels[-1].order

    @property
    def dimension(self):
        return self.__armodels[-1].dimension

    def __normals_block(self, epoch_count, row, column):
        """Block (row, column), row <= column, of the constraint normals of `epoch_count` epochs (grates/lstsq.py:333-362).
        The reference scans all epoch_count - p window positions; only those with column - p <= index <= row contribute."""
        N = _zeros((self.dimension, self.dimension))
        p = self.maximum_order
        for index in range(max(0, column - p), min(row, epoch_count - p - 1) + 1):
            engine.axpby(1.0, self.__armodels[-1]._normal_equation_block_device(row - index, column - index), 1.0, N)
        for order in range(p):
            if row <= order and column <= order:
                engine.axpby(1.0, self.__armodels[order]._normal_equation_block_device(row, column), 1.0, N)
        return N

    def normal_equations(self, epoch_count):
        """Block-banded inverse covariance matrix of `epoch_count` epochs with zero right-hand side (grates/lstsq.py:364-392).
        Interior blocks are equal sums; they are formed once and copied."""
        parameter_count = epoch_count * self.dimension
        block_index = np.arange(0, parameter_count + self.dimension, self.dimension, dtype=int)
        normals_matrix = BlockMatrix(block_index, block_index)
        right_hand_side = np.zeros((parameter_count, 1))
        p = self.maximum_order
        interior = {}
        for row in range(epoch_count):
            for column in range(row, min(epoch_count, row + p + 1)):
                if p <= row <= epoch_count - p - 1:          # full window range, no start-up models: depends on the lag only
                    lag = column - row
                    if lag not in interior:
                        interior[lag] = self.__normals_block(epoch_count, row, column)
                    normals_matrix._set_device(row, column, interior[lag].clone())
                else:
                    normals_matrix._set_device(row, column, self.__normals_block(epoch_count, row, column))
        return NormalEquations(normals_matrix, right_hand_side, 0.0, parameter_count)

    def covariance_function(self, maximum_lag):
        """grates/lstsq.py:394-411"""
        epochs = max(maximum_lag, self.maximum_order) + 1
        system = self.normal_equations(epochs)
        system.compute_covariance(sparse=False)                # full inverse: block (0, k) is the covariance of lag k
        return [system.matrix[0, lag] for lag in range(maximum_lag + 1)]


MAX_WHITENING_ORDER = 128      # of shg_whiten_rows: the halo of a tile of its kernel
MAX_COVARIANCE_ORDER = 4095    # of shg_whiten_rows_long: the longest filter of a CovarianceFunction


class CovarianceFunction:
    """
    Stationary scalar noise given by its covariance function c_0 .. c_q, as a noise model of the observations along the series of
    points (host, NumPy only; no reference counterpart).  Accepted wherever an AutoregressiveModelSequence is: ColouredNoise,
    ArcParameters(noise_model=), the noise_model keyword of NormalEquations.from_accelerations, decorrelate, and through them
    RadialBasisParameters, TemporalParameters and every PostFit.of_*.

    covariance_function holds the lags 0 .. q, 0 <= q <= MAX_COVARIANCE_ORDER: a one-dimensional array, or a sequence of [1, 1]
    arrays as AutoregressiveModelSequence.from_covariance_function takes and PostFit.covariance_function returns.  An arc of up to
    q + 1 points is decorrelated with its full covariance matrix, W = inv(cholesky(Toeplitz(c_0 .. c_(n-1)))); a longer arc with
    that of its first q + 1 points and the AR(q) continuation beyond, the banded W with W^T W the inverse covariance matrix of the
    AR(q) process that matches c_0 .. c_q.  taps() is the table of whitening_taps, built by a Levinson-Durbin recursion in O(q^2):
    the same numbers as whitening_taps(AutoregressiveModelSequence.from_covariance_function(...)) up to rounding, without the
    q + 1 AR models.  Up to q = 128 the filter runs on shg_whiten_rows, bitwise as an AR sequence with these taps; above, on
    shg_whiten_rows_long.

    ValueError for lags that are not finite, c_0 <= 0, q above the limit, [d, d] lags with d != 1, and a function that is not
    positive definite: the order at which the prediction-error variance stops being finite and positive is named.
    """

    def __init__(self, covariance_function):
        try:
            lags = [np.asarray(lag, dtype=np.float64) for lag in covariance_function]
        except (TypeError, ValueError):
            lags = []
        if not lags or not all(lag.shape in ((), (1,)) or (lag.ndim == 2 and lag.shape[0] == lag.shape[1]) for lag in lags):
            raise ValueError('covariance_function must hold the lags 0 .. q: a one-dimensional array or a sequence of [1, 1] arrays')
        for lag in lags:
            if lag.ndim == 2 and lag.shape != (1, 1):
                raise ValueError('covariance function of dimension {0}: only scalar noise (dimension 1) decorrelates an arc'.format(lag.shape[0]))
        c = np.array([float(lag.reshape(())) for lag in lags])
        q = c.size - 1
        if q > MAX_COVARIANCE_ORDER:
            raise ValueError('maximum order {0} of the covariance function above {1}'.format(q, MAX_COVARIANCE_ORDER))
        if not np.all(np.isfinite(c)):
            raise ValueError('the covariance function is not finite at lag {0}'.format(int(np.flatnonzero(~np.isfinite(c))[0])))
        if not c[0] > 0.0:
            raise ValueError('variance c_0 = {0} of the covariance function is not positive'.format(c[0]))
        self.__lags = c
        self.__taps = self.__levinson(c)

    @staticmethod
    def __levinson(c):
        """h [q + 1, q + 1]: row s holds 1 / sigma_s and -phi_k / sigma_s of the best linear predictor of order s"""
        q = c.size - 1
        taps = np.zeros((q + 1, q + 1))
        phi, variance = np.zeros(0), c[0]
        taps[0, 0] = 1.0 / np.sqrt(variance)
        for s in range(1, q + 1):
            reflection = (c[s] - np.dot(phi, c[s - 1:0:-1])) / variance
            phi = np.concatenate((phi - reflection * phi[::-1], (reflection,)))
            variance = variance * (1.0 - reflection * reflection)
            if not (np.isfinite(variance) and variance > 0.0):
                raise ValueError('prediction-error variance {0} at order {1} is not finite and positive: the covariance function is not '
                                 'positive definite there'.format(variance, s))
            sigma = np.sqrt(variance)
            taps[s, 0] = 1.0 / sigma
            taps[s, 1:s + 1] = -phi / sigma
        return taps

    @property
    def maximum_order(self):
        return self.__lags.size - 1

    @property
    def dimension(self):
        return 1

    @property
    def covariance_function(self):
        """the lags 0 .. q as given, ndarray [q + 1]"""
        return self.__lags.copy()

    def taps(self):
        """ndarray [q + 1, q + 1] in the layout of whitening_taps: h[s][0] = 1 / sigma_s, h[s][k] = -phi_k / sigma_s, zero beyond"""
        return self.__taps.copy()


def _covariance_taps(noise_model):
    """whitening_taps of one CovarianceFunction or a list of them; None for anything else"""
    if isinstance(noise_model, CovarianceFunction):
        return noise_model.taps()[None]
    functions = noise_model
    if not isinstance(functions, list) or not functions or not all(isinstance(function, CovarianceFunction) for function in functions):
        return None
    orders = sorted(set(function.maximum_order for function in functions))
    if len(orders) != 1:
        raise ValueError('the noise models of the components differ in their maximum order: {0}'.format(orders))
    return np.stack([function.taps() for function in functions])


def _check_model_orders(sequence):
    """q of an AutoregressiveModelSequence whose models have the orders 0, 1, ..., q <= MAX_WHITENING_ORDER; ValueError else"""
    q = len(sequence.models) - 1
    if q < 0:
        raise ValueError('a noise model without AR models')
    if q > MAX_WHITENING_ORDER:
        raise ValueError('maximum order {0} of the noise model above {1}'.format(q, MAX_WHITENING_ORDER))
    for s, model in enumerate(sequence.models):
        if model.order != s:
            raise ValueError('model {0} of the sequence has order {1}: expected the orders 0, 1, ..., {2}'.format(s, model.order, q))
    return q


def whitening_taps(noise_model):
    """
    Tap rows of the decorrelation filter of scalar AR model sequences, ndarray [C, q + 1, q + 1] (host, NumPy only): row s of a
    sequence is h[s][0] = 1 / sigma_s, h[s][k] = -phi_k / sigma_s (1 <= k <= s) from the coefficients phi and the white-noise
    variance sigma_s^2 of its model of order s, zero beyond.  Applied with the exact start-up of an arc (order 0 for its first
    point, order 1 for the second, ..., stationary from point q + 1 on) the rows form the lower-triangular banded W with
    W^T W = Sigma^-1 = noise_model.normal_equations(L).

    noise_model is one AutoregressiveModelSequence (shared by all components, C = 1) or a sequence of them, one per component in
    the component order of the observations.  ValueError for a model of dimension other than 1, sequences of differing maximum
    order, an order above 128, models that are not of orders 0, 1, ..., q, and a variance that is not finite and positive.

    One CovarianceFunction, or a sequence of them of equal order, one per component, gives their stacked taps() instead, of orders
    up to MAX_COVARIANCE_ORDER.  A sequence that mixes the two types is refused.
    """
    if not isinstance(noise_model, (AutoregressiveModelSequence, CovarianceFunction, list)):
        try:
            noise_model = list(noise_model)                # once: it may be an iterator
        except TypeError:
            pass
    if isinstance(noise_model, list) and any(isinstance(model, VectorNoise) for model in noise_model):
        raise ValueError('a VectorNoise couples all components of a point: pass it alone, not in a sequence of models, one per component')
    taps = _covariance_taps(noise_model)
    if taps is not None:
        return taps
    try:
        sequences = [noise_model] if isinstance(noise_model, AutoregressiveModelSequence) else list(noise_model)
    except TypeError:
        sequences = []
    if not sequences or not all(isinstance(sequence, AutoregressiveModelSequence) for sequence in sequences):
        raise ValueError('noise_model must be an AutoregressiveModelSequence or a sequence of them, one per component')
    orders = sorted(set(len(sequence.models) - 1 for sequence in sequences))
    if len(orders) != 1:
        raise ValueError('the noise models of the components differ in their maximum order: {0}'.format(orders))
    for sequence in sequences:
        q = _check_model_orders(sequence)
    taps = np.zeros((len(sequences), q + 1, q + 1))
    for c, sequence in enumerate(sequences):
        for s, model in enumerate(sequence.models):
            if model.dimension != 1:
                raise ValueError('noise model of dimension {0}: only scalar AR models (dimension 1) decorrelate an arc'.format(model.dimension))
            variance = float(np.asarray(model.white_noise_covariance, dtype=np.float64).reshape(()))
            if not (np.isfinite(variance) and variance > 0.0):
                raise ValueError('white-noise variance {0} of the model of order {1} is not finite and positive'.format(variance, s))
            sigma = np.sqrt(variance)
            taps[c, s, 0] = 1.0 / sigma
            for k in range(1, s + 1):
                taps[c, s, k] = -float(np.asarray(model.coefficients[k - 1], dtype=np.float64).reshape(())) / sigma
    return taps


MIN_VECTOR_DIMENSION, MAX_VECTOR_DIMENSION = 2, 6      # of shg_whiten_rows_vector: the components a lane of its kernel holds


class VectorNoise:
    """
    Noise that couples the K components of a point, given by an AutoregressiveModelSequence of dimension K (VAR models of orders
    0, 1, ..., q, as AutoregressiveModelSequence.from_covariance_function builds them from [K, K] lags), as a noise model of the
    observations along the series of points (host, NumPy only; no reference counterpart).  Accepted
    wherever a scalar AutoregressiveModelSequence is: ColouredNoise, ArcParameters(noise_model=), the noise_model keyword of
    NormalEquations.from_accelerations, decorrelate, and through them RadialBasisParameters, TemporalParameters and every
    PostFit.of_*.  A bare sequence of dimension K > 1 stays refused: the joint filter is opted into with this type.

    taps() is the table H [q + 1, q + 1, K, K] of shg_whiten_rows_vector: H[s][0] = R_s^-T and H[s][k] = -R_s^-T B_k^(s) for
    1 <= k <= s, zero beyond, from the coefficients B_k^(s) and the white-noise covariance Q_s = R_s^T R_s (R_s upper triangular) of
    the model of order s.  With the start-up of an arc, stage[t] = min(t - arc start, q),
    y[t] = sum_{k = 0 .. stage[t]} H[stage[t]][k] x[t - k] is the block lower-triangular banded W with
    W^T W = sequence.normal_equations(L); for a sequence from a covariance function Sigma_k = E[x_t x_(t+k)^T], W Sigma_L W^T = I.

    ValueError unless 2 <= K <= 6, the models have the orders 0, 1, ..., q with q <= 128, every coefficient is a finite [K, K]
    matrix and every Q_s is finite, symmetric and positive definite (the order is named).
    """

    def __init__(self, sequence):
        if not isinstance(sequence, AutoregressiveModelSequence):
            raise ValueError('VectorNoise takes one AutoregressiveModelSequence, got {0!r}'.format(type(sequence).__name__))
        models = sequence.models
        q = _check_model_orders(sequence)
        K = int(np.shape(models[0].white_noise_covariance)[0]) if np.ndim(models[0].white_noise_covariance) == 2 else 1
        if not MIN_VECTOR_DIMENSION <= K <= MAX_VECTOR_DIMENSION:
            raise ValueError('vector noise of dimension {0}: expected {1} .. {2} (a scalar model is passed as the sequence itself)'.format(
                K, MIN_VECTOR_DIMENSION, MAX_VECTOR_DIMENSION))
        taps = np.zeros((q + 1, q + 1, K, K))
        for s, model in enumerate(models):
            Q = np.asarray(model.white_noise_covariance, dtype=np.float64)
            # symmetric up to the rounding of the Yule-Walker solve that formed it (from_covariance_function: Q = Sigma_0 - X^T b as a product)
            if Q.shape != (K, K) or not np.all(np.isfinite(Q)) or not np.all(np.abs(Q - Q.T) <= 1e-8 * np.max(np.abs(Q))):
                raise ValueError('white-noise covariance of the model of order {0} is not a finite symmetric [{1}, {1}] matrix'.format(s, K))
            try:
                L = np.linalg.cholesky(np.triu(Q) + np.triu(Q, 1).T)          # the upper triangle, as engine.potrf reads it; Q = L L^T: R = L^T, R^-T = L^-1
            except np.linalg.LinAlgError:
                raise ValueError('white-noise covariance of the model of order {0} is not positive definite'.format(s)) from None
            taps[s, 0] = np.linalg.inv(L)
            for k in range(1, s + 1):
                B = np.asarray(model.coefficients[k - 1], dtype=np.float64)
                if B.shape != (K, K) or not np.all(np.isfinite(B)):
                    raise ValueError('coefficient {0} of the model of order {1} is not a finite [{2}, {2}] matrix'.format(k, s, K))
                taps[s, k] = -taps[s, 0] @ B
        if not np.all(np.isfinite(taps)):
            raise ValueError('the whitening taps of the noise model are not finite')
        self.__sequence, self.__taps = sequence, taps

    @property
    def sequence(self):
        return self.__sequence

    @property
    def dimension(self):
        return int(self.__taps.shape[2])

    @property
    def maximum_order(self):
        return int(self.__taps.shape[0]) - 1

    def taps(self):
        """ndarray [q + 1, q + 1, K, K]: H[s][0] = R_s^-T, H[s][k] = -R_s^-T B_k^(s) (1 <= k <= s), zero beyond"""
        return self.__taps.copy()


def _arc_starts(arcs, count):
    """start indices of the arcs of a series of `count` points, int64 ndarray (None: the single arc [0], no arc without points);
    ValueError unless they are integers, strictly increasing, start at 0 and stay below count"""
    if arcs is None:
        return np.zeros(min(count, 1), dtype=np.int64)
    given = np.asarray(arcs)
    if given.ndim != 1 or given.size == 0 or not (np.issubdtype(given.dtype, np.integer) or np.all(given == np.floor(given))):
        raise ValueError('arcs must be a sequence of integer start indices')
    starts = given.astype(np.int64)
    if starts[0] != 0 or np.any(np.diff(starts) <= 0) or starts[-1] >= count:
        raise ValueError('arcs must start at 0, increase strictly and stay below the {0} points'.format(count))
    return starts


def arc_stages(arcs, count, order):
    """
    The AR order in use at every point of a series of `count` points in arcs, int32 ndarray [count] (host, NumPy only):
    stage[t] = min(t - start of the arc of t, order).  arcs holds the start indices of the arcs (None: the single arc [0]); ValueError
    unless they are integers, strictly increasing, start at 0 and stay below count.  A data gap starts a new arc.
    """
    count, order = int(count), int(order)
    if count < 0 or order < 0:
        raise ValueError('count {0} and order {1} must not be negative'.format(count, order))
    starts = _arc_starts(arcs, count)
    t = np.arange(count, dtype=np.int64)
    since = t - starts[np.searchsorted(starts, t, side='right') - 1] if count else t
    return np.minimum(since, order).astype(np.int32)


class _WhiteningTables:
    """The tables of a noise model for one series of points: taps and stage on the host and, after to_device, on the device; joint:
    the taps are the [q + 1, q + 1, K, K] of a VectorNoise (shg_whiten_rows_vector), else the [C, q + 1, q + 1] of whitening_taps
    (shg_whiten_rows).  The one place that tells the two filters apart: by the type of the model, never by the shape of a table."""

    def __init__(self, noise_model):
        """every ValueError of the model itself: those of a VectorNoise were raised when it was built, a scalar model goes through
        whitening_taps.  stage is filled for a series by _whitening_tables"""
        self.joint = isinstance(noise_model, VectorNoise)
        self.taps = noise_model.taps() if self.joint else whitening_taps(noise_model)
        self.stage = self.device_taps = self.device_stage = None

    def __iter__(self):
        return iter((self.taps, self.stage))                  # taps, stage = _whitening_tables(...): the pair that it returned before

    def to_device(self, device):
        torch = engine.require_gpu()
        self.device_taps, self.device_stage = engine.to_device(self.taps, device), torch.from_numpy(self.stage).to(device)
        return self

    def apply(self, X, start=0, skip=0):
        """W along the last axis of X [..., n], which holds the points start .. start + n; the first skip of them are history only.  Under a
        VectorNoise the rows of X, all axes but the last flattened, are groups of its K components"""
        stage = self.device_stage[start:start + int(X.shape[-1])]
        if self.joint:
            return engine.whiten_rows_vector(X, taps=self.device_taps, stage=stage, skip=skip)
        return engine.whiten_rows(X, taps=self.device_taps, stage=stage, channels=int(self.taps.shape[0]), skip=skip)


def _whitening_tables(noise_model, arcs, count, components):
    """the _WhiteningTables of a from_* call or of decorrelate, on the host; ValueError before anything reaches the device"""
    tables = _WhiteningTables(noise_model)
    taps, joint = tables.taps, tables.joint
    if joint and taps.shape[2] != components:
        raise ValueError('a VectorNoise of dimension {0} for observations of {1} component{2}: the two must be equal'.format(
            taps.shape[2], components, '' if components == 1 else 's'))
    if not joint and taps.shape[0] not in (1, components):
        raise ValueError('{0} noise models for {1} components: expected one, or one per component'.format(taps.shape[0], components))
    tables.stage = arc_stages(arcs, count, taps.shape[0 if joint else 1] - 1)
    return tables


def decorrelate(values, noise_model, arcs=None):
    """
    W values along the point axis, on the device (shg_whiten_rows): values [M] or [M, K] (host array or device tensor; the result
    has the same kind and shape), noise_model and arcs as in NormalEquations.from_accelerations.  What the normals of a whitened
    adjustment see of the observations; residuals A x^ - l go through it the same way.  A VectorNoise of dimension K whitens the K
    components of values [M, K] jointly (shg_whiten_rows_vector).
    """
    shape = tuple(int(size) for size in values.shape)
    if len(shape) not in (1, 2):
        raise ValueError('values must have shape (M,) or (M, K), got {0}'.format(shape))
    M, K = shape[0], (shape[1] if len(shape) == 2 else 1)
    tables = _whitening_tables(noise_model, arcs, M, K)
    x = engine.to_device(values).reshape(M, K).t().contiguous()
    y = tables.to_device(x.device).apply(x)
    return _like_input(y.t().reshape(shape).contiguous(), values)


MAX_ARC_PARAMETERS = 16        # of shg_segment_products: the accumulators of a wave of its kernel


def arc_basis(arcs, count, degree=1, periods=(), times=None):
    """
    Basis of the parameters that last one arc, ndarray [count, u'] (host, NumPy only), for ArcParameters: the Legendre polynomials
    P_0 .. P_degree of the arc-normalised time tau in [-1, 1] (tau = -1 at the first point of an arc, 1 at its last, 0 for an arc of one
    point; degree=None: no polynomial columns), then cos(2 pi t / period) and sin(2 pi t / period) for every period.  t is `times`
    [count] (finite, the periods in its unit) or else the sample index (the periods in samples).  arcs as in arc_stages.  Degree 1
    is a bias and a drift; a period of one revolution gives the empirical once-per-revolution terms.  ValueError for arcs that
    arc_stages refuses, a negative degree, a period that is not finite and positive, times of another shape or not finite, no column
    at all and more than 16 columns.
    """
    count = int(count)
    if count < 0:
        raise ValueError('count {0} must not be negative'.format(count))
    starts = _arc_starts(arcs, count)
    if degree is not None and (int(degree) != degree or degree < 0):
        raise ValueError('degree must be a non-negative integer or None, got {0!r}'.format(degree))
    polynomials = 0 if degree is None else int(degree) + 1
    periods = np.asarray(periods, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(periods) & (periods > 0)):
        raise ValueError('periods must be finite and positive')
    columns = polynomials + 2 * periods.size
    if columns < 1 or columns > MAX_ARC_PARAMETERS:
        raise ValueError('{0} columns of the arc basis: expected 1 .. {1}'.format(columns, MAX_ARC_PARAMETERS))
    if times is None:
        t = np.arange(count, dtype=np.float64)
    else:
        t = np.asarray(times, dtype=np.float64)
        if t.shape != (count,) or not np.all(np.isfinite(t)):
            raise ValueError('times must be {0} finite values'.format(count))
    basis = np.empty((count, columns))
    if polynomials:
        tau = np.zeros(count)
        for first, last in zip(starts, np.append(starts[1:], count)):
            span = t[last - 1] - t[first]
            if span != 0:
                tau[first:last] = 2.0 * (t[first:last] - t[first]) / span - 1.0
        basis[:, :polynomials] = np.polynomial.legendre.legvander(tau, polynomials - 1)
    for i, period in enumerate(periods):
        basis[:, polynomials + 2 * i] = np.cos(2.0 * np.pi * t / period)
        basis[:, polynomials + 2 * i + 1] = np.sin(2.0 * np.pi * t / period)
    return basis


def frame_basis(basis, frames):
    """
    A per-axis instrument parameter seen in Earth-fixed axes, ndarray [M, 3, 3 u'] (host, NumPy only), the general form of the basis
    of ArcParameters: basis [M, u'] (arc_basis), frames [M, 3, 3] with the instrument axes of every point as rows (as in
    from_gradients).  Column 3 i + a of component k is basis[:, i] * frames[:, a, k]: parameter i of instrument axis a.  ValueError
    for other shapes and for 3 u' > 16.
    """
    basis, frames = np.asarray(basis, dtype=np.float64), np.asarray(frames, dtype=np.float64)
    if basis.ndim != 2 or basis.shape[1] < 1:
        raise ValueError('basis must have shape (M, u), got {0}'.format(basis.shape))
    if frames.shape != (basis.shape[0], 3, 3):
        raise ValueError('frames must have shape ({0}, 3, 3), got {1}'.format(basis.shape[0], frames.shape))
    if 3 * basis.shape[1] > MAX_ARC_PARAMETERS:
        raise ValueError('{0} columns of the frame basis: expected at most {1}'.format(3 * basis.shape[1], MAX_ARC_PARAMETERS))
    return np.einsum('ti,tak->tkia', basis, frames).reshape(basis.shape[0], 3, 3 * basis.shape[1])


def component_basis(basis, components):
    """
    The shared basis [M, u'] of ArcParameters written in its general form, ndarray [M, K, K u'] (host, NumPy only), block-diagonal in
    the K = components components: column c u' + j of component c is basis[:, j], every other column of that component is zero, so
    every component has u' parameters of its own as under the shared form, and parameters(x) of the result is [arcs, K u'] with the
    parameter index c u' + j.  What a VectorNoise needs in place of the shared form, whose components its joint filter couples.
    ValueError for other shapes, K < 1 and K u' > 16.
    """
    basis, K = np.asarray(basis, dtype=np.float64), int(components)
    if basis.ndim != 2 or basis.shape[1] < 1:
        raise ValueError('basis must have shape (M, u), got {0}'.format(basis.shape))
    if K < 1:
        raise ValueError('components must be positive, got {0}'.format(components))
    u = basis.shape[1]
    if K * u > MAX_ARC_PARAMETERS:
        raise ValueError('{0} columns of the component basis: expected at most {1}'.format(K * u, MAX_ARC_PARAMETERS))
    general = np.zeros((basis.shape[0], K, K * u))
    for c in range(K):
        general[:, c, c * u:(c + 1) * u] = basis
    return general


def _arc_reduction(G, b):
    """Host part of the elimination of arc-wise parameters: G [units, u, u] and b [units, u] of the units (arcs, or arcs and
    channels) -> R [units, u, u] with the columns V_keep Lambda_keep^-1/2 of numpy.linalg.eigh(G) (eigenvalues above 1e-12 of the
    largest; zero columns for the dropped directions, all of them where the largest is not positive), R^T b [units, u] and the ranks."""
    units, u = b.shape
    R, ranks = np.zeros((units, u, u)), np.zeros(units, dtype=np.int64)
    for i in range(units):
        values, vectors = np.linalg.eigh(G[i])
        if not values[-1] > 0.0:
            continue
        kept = values > 1e-12 * values[-1]
        ranks[i] = np.count_nonzero(kept)
        R[i][:, kept] = vectors[:, kept] / np.sqrt(values[kept])
    return R, np.einsum('ijr,ij->ir', R, b), ranks


class _Observations:
    """The observations of one from_* or of_* call, as _observations checked them on the host: the degrees, P, M, K and the weights with
    their layout (engine.check_observation_weights).  The per-point arguments stay as the call gave them until to_device; take(order)
    puts them in another order of the points before that.  to_device, after every other check of the call, fills l [M, K], the
    observations times root, root = sqrt(w) [M, K] or [M, 1] (None without weights) and design_block(first, last), the transposed design
    matrix [P, K, Mb] (or [P, Mb]) of the points first .. last, scaled alike: the design call of the kind (engine.OBSERVATION_KINDS) on
    the slice of every per-point tensor and of the weights."""

    def __init__(self, kind, arguments, band, M, K, layout, extra):
        self.min_degree, self.max_degree, self.P = band.min_degree, band.max_degree, (band.max_degree + 1) ** 2 - band.min_degree ** 2
        self.M, self.K, self.weights, self.layout = M, K, arguments['weights'], layout
        self.__kind, self.__arguments, self.__band, self.__extra = kind, arguments, band, extra
        self.l = self.root = self.design_block = None

    def take(self, order):
        per_point = {name: _take(self.__arguments[name], order) for name in self.__kind.points + ('weights',)}
        self.__arguments, self.weights = dict(self.__arguments, **per_point), per_point['weights']

    def to_device(self):
        torch = engine.require_gpu()
        kind, band, extra = self.__kind, self.__band, self.__extra
        tensors = engine.upload_observations(kind, self.__arguments)
        l, w = kind.values(tensors.pop(kind.observed), extra), tensors['weights']
        design = kind.design if band.basis is None else kind.rbf_design
        self.design_block = lambda first, last: design(band, {name: None if t is None else t[first:last] for name, t in tensors.items()}, extra)
        self.root = torch.sqrt(w if self.layout == 2 else w[:, None]) if self.layout else None
        self.l = l * self.root if self.layout else l


def _observations(kind, arguments, band):
    """The record of the observations of a from_* or of_* call: kind names an entry of engine.OBSERVATION_KINDS, arguments is the dict of
    its per-point arguments, options and weights, band an engine.Band.  check_degrees, then the checks of the kind; with a basis the
    parameters are the node values of that gravityfield.RadialBasisFunctions instead of the coefficients, so P is its node count, and
    the degrees and constants of the call must be the basis's (ValueError otherwise, as for an anisotropic basis).  All of it on the
    host."""
    kind = engine.OBSERVATION_KINDS[kind]
    min_degree, max_degree = engine.check_degrees(band.min_degree, band.max_degree)
    observations = _Observations(kind, arguments, band._replace(min_degree=min_degree, max_degree=max_degree), *kind.check(arguments))
    basis = band.basis
    if basis is not None:
        for name, given, own in (('min_degree', min_degree, int(basis.min_degree)), ('max_degree', max_degree, int(basis.max_degree)),
                                 ('GM', float(band.GM), float(basis.GM)), ('R', float(band.R), float(basis.R))):
            if given != own:
                raise ValueError('{0} of the call is {1!r} but the basis has {2!r}: pass the values of the basis'.format(name, given, own))
        basis.degree_factors
        observations.P = int(basis.point_distribution.longitude.size)
    return observations


def _route(kind, arguments, band, model, block_points, temporal=None, fit=None):
    """Every public from_* and of_*: the observations of the kind, under model (None, a ColouredNoise, an ArcParameters or a
    _StochasticModel), in blocks of block_points; temporal is the TemporalParameters of the call, whose _Windows puts the points in
    its order before the upload, fit the PostFit of an of_* call.  Returns the NormalEquations, or the PostFit after its pass."""
    observations, model = _observations(kind, arguments, band), _StochasticModel.of(model)
    windows = None if temporal is None else _Windows(temporal, observations)
    if fit is None:
        return NormalEquations._normals(observations, model, block_points, windows)
    return fit._pass(observations, model, block_points, windows)


class _StochasticModel:
    """The stochastic model of one from_* or of_* call beyond the weights: noise_model and arcs as NormalEquations.from_accelerations
    takes them, parameters an ArcParameters or None; of(model) reads them from None, a ColouredNoise or an ArcParameters.  check(M, K)
    fills whitening, the _WhiteningTables of the call on the host (None without a noise model), and starts, the start indices of the
    arcs; to_device uploads them and fills halo, the host's stage table: what a block takes along in front."""

    def __init__(self, noise_model=None, arcs=None, parameters=None):
        self.noise_model, self.arcs, self.parameters = noise_model, arcs, parameters
        self.whitening = self.starts = self.halo = None

    @classmethod
    def of(cls, model):
        if isinstance(model, cls):
            return model
        if isinstance(model, _BoundModel):
            return cls(model.noise_model, model.arcs, model if isinstance(model, ArcParameters) else None)
        if model is None:
            return cls()
        raise ValueError('model must be None, a ColouredNoise or an ArcParameters (arcs belong to one of them), got {0!r}'.format(model))

    def check(self, M, K):
        """ValueError for what _whitening_tables refuses, arcs that belong to nothing and a basis that is neither [M, u'] nor [M, K, u]"""
        if self.noise_model is not None:
            self.whitening = _whitening_tables(self.noise_model, self.arcs, M, K)
        elif self.arcs is not None and self.parameters is None:
            raise ValueError('arcs are those of the noise model: pass noise_model as well')
        self.starts = _arc_starts(self.arcs, M)
        if self.parameters is not None:
            shape = self.parameters.basis.shape
            if shape[0] != M or (len(shape) == 3 and shape[1] != K):
                raise ValueError('the arc basis must have shape ({0}, u) or ({0}, {1}, u), got {2}'.format(M, K, shape))
            if self.whitening is not None and self.whitening.joint and len(shape) == 2:
                raise ValueError('a shared arc basis ({0}, u) gives every component parameters of its own, which a VectorNoise couples: pass the '
                                 'general basis lstsq.component_basis(basis, {1}) of shape ({0}, {1}, {1} u)'.format(M, K))

    def to_device(self, device):
        if self.whitening is not None:
            self.halo = self.whitening.to_device(device).stage


def _prepare(observations, model, block_points, fit=None, windows=None):
    """Every from_* and of_* call between the checks of its observations and its pass: block_points as a positive int (None: the default),
    the model, the solution and the vectors of a PostFit and, under TemporalParameters, the blocks of the call's _Windows, every
    ValueError before anything reaches the device; then the uploads."""
    default = NormalEquations.default_block_points if windows is None else windows.default_block_points
    block_points = int(default(observations.P, observations.K) if block_points is None else block_points)
    if block_points < 1:
        raise ValueError('block_points must be positive, got {0}'.format(block_points))
    model.check(observations.M, observations.K)
    if fit is not None:
        fit._check(observations.P if windows is None else windows.B * observations.P)
    if windows is not None:
        windows.plan(model, block_points)
    observations.to_device()
    model.to_device(observations.l.device)
    if windows is not None:
        windows.to_device(observations.l.device)
    return block_points


def _design_blocks(observations, model, block_points):
    """The blocks of the from_* classmethods and of PostFit, one after the other: (first, last, At [P, K Mb], lb [K Mb, 1], plain, skip)
    of the points first .. last of the observations l [M, K].  Without a noise model At is design_block(first, last) and lb the
    observations, component-major as the columns of At; plain is At and skip 0.  With one a block takes the skip = stage[first]
    points in front of it along (none where it starts an arc), shg_whiten_rows turns the design matrix and the observations of
    first - skip .. last into those of W A and W l at first .. last in a second buffer, and plain [P, K (skip + Mb)] is the design matrix
    as design_block gave it."""
    P, M, K, l = observations.P, observations.M, observations.K, observations.l
    for first in range(0, M, block_points):
        last = min(first + block_points, M)
        if model.whitening is None:
            At = observations.design_block(first, last).reshape(P, K * (last - first))
            yield first, last, At, l[first:last].t().reshape(-1, 1), At, 0      # component-major, as the columns of At
        else:
            start = first - int(model.halo[first])
            plain = observations.design_block(start, last).reshape(P * K, last - start)
            At = model.whitening.apply(plain, start, first - start).reshape(P, K * (last - first))
            lb = model.whitening.apply(l[start:last].t().contiguous(), start, first - start).reshape(-1, 1)
            yield first, last, At, lb, plain.reshape(P, K * (last - start)), first - start


def _mirror_upper(N):
    """the upper triangle of N [P, P], of which both were computed, onto the lower one: N is exactly symmetric afterwards"""
    N.triu_()
    N.add_(engine._torch().triu(N, 1).t())


MAX_TEMPORAL_SLOTS = engine.WINDOW_SLOTS      # of shg_window_expand: the fields one block of points may span

_TemporalBlock = collections.namedtuple('_TemporalBlock', 'start first last field slots run_slot run_begin supports')


def temporal_blocks(first, W, block_points, stage=None):
    """
    The blocks of a from_* or of_* call under TemporalParameters (host, NumPy only): first [M] are the window
    starts of the points in the order of the call, W the fields per window, stage [M] the history every point takes along under a
    noise model (arc_stages), None without one.  A block is a _TemporalBlock: it owns the points first .. last - 1, reads start =
    first - stage[first] .. last - 1 (n columns, the first `skip` = first - start of them history only), spans the fields `field` ..
    field + slots - 1 with slots = E = (largest - smallest window start of its n points) + W <= 16, and carries run_slot / run_begin, the
    runs of columns with one window start as shg_window_expand takes them (slots relative to `field`).  supports[e] is the range
    (c0, c1) of owned columns, counted from `first`, outside of which slot e of the whitened expanded block is structurally zero --
    column t is inside when one of the points t - stage[t] .. t holds the slot in its window -- or None where no owned column does.

    Without a noise model `first` must not decrease (the caller sorts: the normals are permutation-invariant); blocks are cut at
    every change of the window start and restart at the first point of a run, so E = W and no zero is multiplied.  With one the order
    of the points is kept; a block ends early where one more point would need more than 16 slots, and where a change of the window
    start meets the start of an arc (nothing crosses it, so the blocks behind it are those of a call on those points alone).
    ValueError where a single point with its history spans more than 16 slots.
    """
    first, W, block_points = np.asarray(first, dtype=np.int64), int(W), int(block_points)
    M = int(first.shape[0])
    if stage is None and M > 1 and bool(np.any(first[1:] < first[:-1])):
        raise ValueError('without a noise model the window starts must not decrease: sort the points (engine.points_at_plan)')
    halo = np.zeros(M, dtype=np.int64) if stage is None else np.asarray(stage, dtype=np.int64)
    blocks, t = [], 0
    while t < M:
        start = t - int(halo[t])
        end = min(t + block_points, M)
        window = first[start:end]
        if stage is None:
            change = np.flatnonzero(window[1:] != window[0])
            if change.size:
                end = t + 1 + int(change[0])
        else:
            span = np.maximum.accumulate(window) - np.minimum.accumulate(window) + W
            if span[t - start] > MAX_TEMPORAL_SLOTS:
                raise ValueError('point {0} and its history of {1} points span {2} fields: at most {3} fit one block'.format(
                    t, t - start, int(span[t - start]), MAX_TEMPORAL_SLOTS))
            over = np.flatnonzero(span[t - start:] > MAX_TEMPORAL_SLOTS)
            if over.size:
                end = t + int(over[0])
            cut = np.flatnonzero((halo[t + 1:end] == 0) & (first[t + 1:end] != first[t:end - 1]))
            if cut.size:
                end = t + 1 + int(cut[0])
        blocks.append(_temporal_block(first, halo, W, start, t, end))
        t = end
    return blocks


def _temporal_block(first, halo, W, start, own, end):
    """the _TemporalBlock of the points own .. end - 1 with the history start .. own - 1"""
    window = first[start:end]
    field = int(window.min())
    local, slots = window - field, int(window.max()) - field + W
    n, skip = end - start, own - start
    runs = np.flatnonzero(np.concatenate(([True], local[1:] != local[:-1])))
    columns, reach = np.arange(skip, n), halo[start + skip:end]
    supports = []
    for e in range(slots):
        held = np.concatenate(([0], np.cumsum((local <= e) & (e < local + W))))
        inside = np.flatnonzero(held[columns + 1] - held[columns - reach] > 0)
        supports.append((int(inside[0]), int(inside[-1]) + 1) if inside.size else None)
    return _TemporalBlock(start, own, end, field, slots, local[runs].astype(np.int32), np.concatenate((runs, [n])).astype(np.int32), supports)


def temporal_pattern(blocks):
    """the set of (f, f'), f <= f', of the blocks of the normal matrix that the blocks of temporal_blocks touch: the pairs of slots of one
    block whose supports intersect.  Host only."""
    pattern = set()
    for block in blocks:
        for a, b, _, _ in _slot_pairs(block):
            pattern.add((block.field + a, block.field + b))
    return pattern


def _slot_pairs(block):
    """(a, b, c0, c1) of the pairs of slots a <= b of a block whose supports intersect in the columns c0 .. c1 - 1"""
    for a in range(block.slots):
        for b in range(a, block.slots):
            if block.supports[a] is not None and block.supports[b] is not None:
                c0, c1 = max(block.supports[a][0], block.supports[b][0]), min(block.supports[a][1], block.supports[b][1])
                if c0 < c1:
                    yield a, b, c0, c1


def _temporal_design_blocks(observations, model, windows):
    """The blocks of a call under TemporalParameters, one after the other: (block, S~ [E, P, K Mb], lb [K Mb, 1], S [E, P, K n], skip).
    The transposed design matrix T [P, K, n] of the points block.start .. block.last, as design_block gives it (scaled by sqrt(w)), is
    expanded to the E slots of the block by shg_window_expand, S[e] = factor * T inside the window of a point and +0.0 outside; only
    then shg_whiten_rows mixes neighbouring points, which have different factors, into S~ of the points block.first .. block.last (the
    row index of S ends in the component, so row % K is the channel).  Without a noise model S~ is S and skip 0."""
    P, K, l = observations.P, observations.K, observations.l
    for block in windows.blocks:
        start, first, last, E = block.start, block.first, block.last, block.slots
        n = last - start
        T = observations.design_block(start, last).reshape(P * K, n)
        S = engine.window_expand(T, windows.device_factors[start:last], block.run_slot, block.run_begin, E).reshape(E, P, K * n)
        if model.whitening is None:
            yield block, S, l[first:last].t().reshape(-1, 1), S, 0
        else:
            St = model.whitening.apply(S.reshape(E * P * K, n), start, first - start).reshape(E, P, K * (last - first))
            lb = model.whitening.apply(l[start:last].t().contiguous(), start, first - start).reshape(-1, 1)
            yield block, St, lb, S, first - start


def _temporal_pass_blocks(observations, model, windows):
    """_temporal_design_blocks as PostFit._pass reads _design_blocks, with the columns of the solution that a block sees behind: the
    field-major order makes the window of a block one contiguous slice"""
    P = observations.P
    for block, St, lb, S, skip in _temporal_design_blocks(observations, model, windows):
        E = block.slots
        yield block.first, block.last, St.reshape(E * P, -1), lb, S.reshape(E * P, -1), skip, slice(block.field * P, (block.field + E) * P)


class _ArcSetup:
    """What the elimination of arc-wise parameters and the post-fit pass share of an ArcParameters, from observations and a model on the
    device.  The basis goes the way of the design matrix (times root, then W) into Bt [u, K, M] (plain=True keeps the one before W as
    plain_Bt), once; shg_segment_products gives G_a = B_a^T B_a and b_a = B_a^T l_a of all arcs (summed over the components for the general
    form, Kc = 1; Kc = K for a shared basis), the host R_a = V Lambda^-1/2 of the kept eigenpairs of G_a, g = R^T b and the ranks
    (_arc_reduction; R_d and g_d on the device).  seg holds the boundaries of the arcs on the device, bounds on the host."""

    def __init__(self, observations, model, plain=False):
        torch = engine.require_gpu()
        l, root, M, K = observations.l, observations.root, observations.M, observations.K
        basis = engine.to_device(model.parameters.basis, l.device)
        self.shared = basis.dim() == 2
        Bt = basis.t()[:, None, :].expand(-1, K, -1) if self.shared else basis.permute(2, 1, 0)
        Bt = (Bt if root is None else Bt * root.expand(M, K).t()[None]).contiguous()                    # [u, K, M]
        lt = l.t().contiguous()
        self.plain_Bt = Bt if plain else None
        if model.whitening is not None:
            Bt, lt = model.whitening.apply(Bt), model.whitening.apply(lt)
        self.Bt, self.u, self.Kc = Bt, int(Bt.shape[0]), (K if self.shared else 1)
        self.bounds = np.append(model.starts, M)
        self.arcs = len(self.bounds) - 1
        self.seg = torch.from_numpy(self.bounds.astype(np.int32)).to(l.device)
        G = engine.segment_products(Bt, Bt, self.seg, channels=K).permute(2, 1, 0, 3)                    # [arcs, K, u, u]
        b = engine.segment_products(lt, Bt, self.seg, channels=K).permute(1, 0, 2)                       # [arcs, K, u]
        if not self.shared:
            G, b = G.sum(1, keepdim=True), b.sum(1, keepdim=True)
        units = self.arcs * self.Kc
        self.R, self.g, self.ranks = _arc_reduction(engine.to_host(G).reshape(units, self.u, self.u), engine.to_host(b).reshape(units, self.u))
        self.R_d, self.g_d = engine.to_device(self.R, l.device), engine.to_device(self.g, l.device).reshape(-1, 1)


class ArcElimination:
    """
    What NormalEquations keeps of the elimination of its arc-wise parameters (ne.arc_elimination; ArcParameters): `ranks`, the number of
    directions eliminated per arc (ndarray [arcs], or [arcs, K] for a shared basis), and their sum `count`, by which
    observation_count was reduced.  parameters(solution) returns the parameters y_a = R_a (R_a^T b_a - D_a^T x) that belong to a
    solution x of the reduced system, as a host ndarray [arcs, K, u'] (shared basis) or [arcs, u], zero along the dropped
    directions.  It needs the D_a, which ArcParameters(keep=True) retains on the device: P K u' doubles per arc (shared basis),
    P u for the general form.
    """

    def __init__(self, ranks, R, g, shared, columns):
        self.ranks = ranks
        self.count = int(ranks.sum())
        self.__R, self.__g, self.__shared, self.__columns, self.__merged = R, g, shared, columns, None

    def parameters(self, solution):
        if self.__columns is None:
            raise ValueError('the parameters of the arcs need the eliminated columns: build with ArcParameters(keep=True)')
        x = _dev(solution).reshape(-1, 1)
        products = [engine.to_host(engine.gemm(D, x, transa=True)) for D in self.__columns]
        y = self.__g - np.concatenate(products).reshape(self.__g.shape)
        y = np.einsum('akjr,akr->akj', self.__R, y)
        return y if self.__shared else y[:, 0]

    def _columns(self):
        """the kept D_a = C_a R_a of all arcs side by side, [P, arcs Kc u] on the device (arc-major, then the component of a shared
        basis, then the direction), or None after ArcParameters(keep=False): what PostFit.leverages reduces the rows with"""
        if self.__columns is None or not self.__columns:
            return None
        if self.__merged is None:                                     # (parameters() keeps its products per block of the sweep)
            self.__merged = self.__columns[0] if len(self.__columns) == 1 else engine._torch().cat(self.__columns, dim=1)
        return self.__merged


class _ArcSweep:
    """The elimination of the arc-wise parameters over the blocks of one from_* call, on its normals and
    right-hand side.  block(first, last, At): shg_segment_products on the whitened At, with the arc boundaries clipped to the block, gives
    the part of C_a = A_a^T B_a that lies in it; an arc that continues past the block keeps its sum in the carry [P, Kc, u], an arc that
    ends gives D_a = C_a R_a, and N -= D D^T, n -= D (R^T b) run as one product each once `update_columns` columns of D are waiting (the
    update reads and writes all of N); flush() applies the rest after the last block, before the mirroring.  keep retains every D."""

    def __init__(self, observations, model, normals, side, update_columns):
        self.setup, self.normals, self.side, self.update_columns = _ArcSetup(observations, model), normals, side, update_columns
        self.carry = _zeros((observations.P, self.setup.Kc, self.setup.u))
        self.columns = [] if model.parameters.keep else None
        self.pending, self.applied, self.finished = [], 0, 0                                              # D of finished arcs not yet subtracted

    def block(self, first, last, At):
        torch = engine.require_gpu()
        s, P = self.setup, int(At.shape[0])
        K, Kc, u = int(s.Bt.shape[1]), s.Kc, s.u
        a0, a1 = int(np.searchsorted(s.bounds, first, side='right')) - 1, int(np.searchsorted(s.bounds, last, side='left')) - 1
        cut = (s.seg[a0:a1 + 2] - first).clamp_(0, last - first)                                         # arcs a0 .. a1 meet the block
        S = engine.segment_products(At.reshape(P * K, last - first), s.Bt[:, :, first:last], cut, channels=K).reshape(P, K, a1 - a0 + 1, u)
        C = S.permute(0, 2, 1, 3) if s.shared else S.sum(1, keepdim=True).permute(0, 2, 1, 3)            # [P, arcs of the block, Kc, u]
        C[:, 0] += self.carry
        ended = a1 - a0 + (1 if s.bounds[a1 + 1] <= last else 0)
        if ended <= a1 - a0:
            self.carry = C[:, ended].clone()
        else:
            self.carry.zero_()
        if ended:
            D = torch.empty((ended * Kc, P, u), dtype=torch.float64, device=At.device)
            engine.gemm_ex(C[:, :ended].permute(1, 2, 0, 3).reshape(ended * Kc, P, u), s.R_d[a0 * Kc:(a0 + ended) * Kc], D)
            D = D.permute(1, 0, 2).reshape(P, ended * Kc * u).contiguous()                               # u = 1: the reshape alone is a strided view
            self.pending.append(D)
            if self.columns is not None:
                self.columns.append(D)
        self.finished = a0 + ended
        if sum(int(D.shape[1]) for D in self.pending) >= self.update_columns:
            self.flush()

    def flush(self):
        if self.pending:
            torch = engine.require_gpu()
            width = self.setup.Kc * self.setup.u
            D = self.pending[0] if len(self.pending) == 1 else torch.cat(self.pending, dim=1)            # the arcs applied .. finished
            engine.gemm(D, D, transb=True, alpha=-1.0, beta=1.0, out=self.normals)
            engine.gemm(D, self.setup.g_d[self.applied * width:self.finished * width], alpha=-1.0, beta=1.0, out=self.side)
            self.pending, self.applied = [], self.finished

    def result(self):
        s = self.setup
        shape = (s.arcs, s.Kc) if s.shared else (s.arcs,)
        return ArcElimination(s.ranks.reshape(shape), s.R.reshape(s.arcs, s.Kc, s.u, s.u), s.g.reshape(s.arcs, s.Kc, s.u), s.shared, self.columns)


class BlockMatrix:
    """
    Sparse rectangular block matrix with device-resident blocks (grates/lstsq.py:414-912).  `matrix[i, j]` returns a host
    copy of a block (None when the block is empty) and `matrix[i, j] = array` stores a device copy; `device_block(i, j)`
    gives the tensor itself.
    """

    def __init__(self, row_index, column_index):
        self.shape = (len(row_index) - 1, len(column_index) - 1)
        self.__row_index = row_index
        self.__column_index = column_index
        self.__data = {}
        self.__inverse_factor = {}      # diagonal index -> inverse of the upper triangular factor block
        self._inverse_in_place = False  # the factorisation keeps U_ii^-1 in the diagonal blocks instead of U_ii (distributed chains)
        self._holds_factor_inverses = False   # ... and has done so: the diagonal blocks currently hold U_ii^-1

    def copy(self):
        """Deep copy of BlockMatrix"""
        output = BlockMatrix(self.__row_index, self.__column_index)
        for key, block in self.__data.items():
            output.__data[key] = block.clone()
        output._inverse_in_place = self._inverse_in_place
        output._holds_factor_inverses = self._holds_factor_inverses
        return output

    def __require_plain_factor(self, operation):
        """A chain factored with `_inverse_in_place` keeps U_ii^-1 where the reference's class keeps U_ii: only the solves and the
        sparse inverse understand that state."""
        if self._holds_factor_inverses:
            raise ValueError('{0}: the diagonal blocks hold the inverses of the factor blocks (in-place factorisation of '
                             'grates_amd.distributed); only solve_triangular and sparse_inverse are defined in this state'.format(operation))

    @staticmethod
    def compute_block_index(array_shape, block_size):
        """grates/lstsq.py:437-463"""
        def bounds(extent):
            # 0, block_size, 2 block_size, ..., extent (the last block may be smaller)
            return np.append(np.arange(0, extent, block_size), extent).astype(int) if extent > 0 else np.array([0])
        return bounds(array_shape[0]), bounds(array_shape[1])

    @staticmethod
    def from_array(array, row_index, column_index):
        """Block matrix from a 2D ndarray; blocks without a non-zero entry stay empty (grates/lstsq.py:466-497)."""
        if not isinstance(array, np.ndarray) or array.ndim != 2:
            raise ValueError('from_array expects a two-dimensional numpy.ndarray')
        for axis, index in enumerate((row_index, column_index)):
            if index[-1] != array.shape[axis]:
                raise ValueError('block index of axis {0} ends at {1}, the array has {2} entries there'.format(axis, index[-1], array.shape[axis]))
        block_matrix = BlockMatrix(row_index, column_index)
        for row in range(len(row_index) - 1):
            for column in range(len(column_index) - 1):
                block = array[row_index[row]:row_index[row + 1], column_index[column]:column_index[column + 1]]
                if np.count_nonzero(block):
                    block_matrix[row, column] = block
        return block_matrix

    def to_array(self):
        """2D ndarray (host) of the whole matrix (grates/lstsq.py:499-514)"""
        array = np.zeros((self.__row_index[-1], self.__column_index[-1]))
        for (row, column), block in self.__data.items():
            array[self.__row_slice(row), self.__column_slice(column)] = engine.to_host(block)
        return array

    def __check_bounds(self, i, j):
        if i > self.shape[0]:
            raise IndexError("block index {0} is out of bounds for axis 0 with size {1}".format(i, self.shape[0]))
        if j > self.shape[1]:
            raise IndexError("block index {0} is out of bounds for axis 1 with size {1}".format(j, self.shape[1]))

    def __block_shape(self, i, j):
        return int(self.__row_index[i + 1] - self.__row_index[i]), int(self.__column_index[j + 1] - self.__column_index[j])

    def __row_slice(self, i):
        return slice(int(self.__row_index[i]), int(self.__row_index[i + 1]), 1)

    def __column_slice(self, i):
        return slice(int(self.__column_index[i]), int(self.__column_index[i + 1]), 1)

    def __check_item(self, i, j, item):
        if not (isinstance(item, np.ndarray) or _is_tensor(item)):
            raise ValueError('Block matrix item must be of type ' + str(np.ndarray))
        if item.ndim != 2:
            raise ValueError('Block matrix item must be a two-dimensional ' + str(np.ndarray))
        if tuple(item.shape) != self.__block_shape(i, j):
            raise ValueError('Block matrix item at position ({0:d}, {1:d}) must be of size ({2:d}, {3:d}). '
                             'Got ({4:d}, {5:d}).'.format(i, j, *self.__block_shape(i, j), item.shape[0], item.shape[1]))

    def __setitem__(self, key, value):
        if not isinstance(key, tuple) and len(key) != 2:
            raise IndexError("Indices to block matrix must be tuples of length 2")
        self.__check_bounds(key[0], key[1])
        self.__check_item(key[0], key[1], value)
        self._set_device(key[0], key[1], _dev(value))

    def _set_device(self, i, j, tensor):
        """store a device tensor as block (i, j); no copy when it is dense row-major (what csrc/blockchol.hip assumes of every block)"""
        self.__data[(int(i), int(j))] = tensor if tensor.is_contiguous() else tensor.contiguous()
        if i == j:
            self.__inverse_factor.pop(int(i), None)

    def __getitem__(self, key):
        if not isinstance(key, tuple) and len(key) != 2:
            raise IndexError("Indices to block matrix must be tuples of length 2")
        self.__check_bounds(key[0], key[1])
        block = self.__data.get((int(key[0]), int(key[1])))
        return None if block is None else engine.to_host(block)

    def _extent(self):
        """(rows, columns) of the whole matrix"""
        return int(self.__row_index[-1]), int(self.__column_index[-1])

    def device_block(self, i, j):
        """device tensor of block (i, j), or None"""
        return self.__data.get((int(i), int(j)))

    def is_nonzero(self, row, column):
        """whether block (row, column) is stored"""
        return (int(row), int(column)) in self.__data

    def __nz(self, i, j):
        return (i, j) in self.__data

    def __matmul__(self, other):
        """C = A B over the non-zero blocks (grates/lstsq.py:651-681)"""
        if not isinstance(other, BlockMatrix):
            raise ValueError('BlockMatrix @ {0} is not defined'.format(type(other).__name__))
        product = BlockMatrix(self.__row_index, other.__column_index)
        inner = range(self.shape[1])
        for i in range(product.shape[0]):
            for j in range(product.shape[1]):
                for k in (k for k in inner if self.__nz(i, k) and other.__nz(k, j)):       # ascending k: upstream summation order
                    engine.gemm(self.__data[(i, k)], other.__data[(k, j)], beta=1.0, out=product.__set_block(i, j))
        return product

    def __set_block(self, i, j):
        """zero block on first use (grates/lstsq.py:683-696)"""
        if (i, j) not in self.__data:
            self.__data[(i, j)] = _zeros(self.__block_shape(i, j))
        return self.__data[(i, j)]

    # ---- numeric kernels: one libshg call per operation (csrc/blockchol.hip walks the blocks on the device) -------------------
    def __square_bounds(self):
        if len(self.__row_index) != len(self.__column_index) or np.any(np.asarray(self.__row_index) != np.asarray(self.__column_index)):
            raise ValueError('operation needs a square block matrix with equal row and column blocks')
        return np.ascontiguousarray(self.__row_index, dtype=np.int32)

    def __block_table(self):
        """the stored upper blocks in compressed row form (engine.BlockTable)"""
        return engine.BlockTable(self.__square_bounds(), self.__data)

    def __inverse_table(self):
        """scratch matrices that hold the inverses of the diagonal factor blocks (kept until a block changes)"""
        nb = self.shape[0]
        table = np.zeros(nb, dtype=np.uint64)
        for i in range(nb):
            if i not in self.__inverse_factor:
                size = self.__block_shape(i, i)[0]
                self.__inverse_factor[i] = self.__data[(i, i)] if self._inverse_in_place else _zeros((size, size))
            table[i] = self.__inverse_factor[i].data_ptr()
        return table

    def __allocate_fill(self):
        """symbolic factorisation: eliminating block row r couples every pair of its off-diagonal blocks (r, c), (r, d), c <= d,
        so block (c, d) of the factor is non-zero as well"""
        nb = self.shape[0]
        pattern = [set() for _ in range(nb)]
        for (i, j) in self.__data:
            if j > i:
                pattern[i].add(j)
        for i in range(nb):
            if not self.__nz(i, i):
                raise np.linalg.LinAlgError('diagonal block {0} of the matrix is empty'.format(i))
        for r in range(nb):
            cols = sorted(pattern[r])
            for a, c in enumerate(cols):
                for d in cols[a:]:
                    if not self.__nz(c, d):
                        self.__data[(c, d)] = _zeros(self.__block_shape(c, d))
                    if d != c:
                        pattern[c].add(d)

    def cholesky(self):
        """
        Cholesky factorization N = W^T W in place; only the upper triangle is referenced, afterwards the matrix holds the
        upper triangular factor W (grates/lstsq.py:698-717).  Raises numpy.linalg.LinAlgError if a diagonal block is not
        positive definite.
        """
        self.__square_bounds()
        self.__allocate_fill()
        self.__inverse_factor.clear()
        pivot = engine.block_potrf(self.__block_table(), self.__inverse_table())
        self._holds_factor_inverses = self._inverse_in_place
        if pivot:
            raise np.linalg.LinAlgError('{0}-th leading minor of the array is not positive definite'.format(pivot))

    def _cholesky_rows(self, first, last):
        """Eliminate the block rows first <= r < last only (shg_block_potrf_rows): the rows from `last` on are left as the Schur
        complement.  A sequence of calls that covers all rows in ascending order equals cholesky()."""
        self.__square_bounds()
        if first == 0:
            self.__allocate_fill()
            self.__inverse_factor.clear()
        pivot = engine.block_potrf(self.__block_table(), self.__inverse_table(), first, last)
        self._holds_factor_inverses = self._inverse_in_place
        if pivot:
            raise np.linalg.LinAlgError('{0}-th leading minor of the array is not positive definite'.format(pivot))

    def _cholesky_rows_pair(self, other, first, last):
        """_cholesky_rows(first, last) of this matrix and of `other` in one pass (shg_block_potrf_rows_pair).  The two matrices
        must have the same structure in the leading block rows and columns that the rows before `last` reach (two chains that
        need not be equally long: up to block `last`; matrices with border columns: all of them)."""
        tables, inverses = [], []
        for m in (self, other):
            m.__square_bounds()
            if first == 0:
                m.__allocate_fill()
                m.__inverse_factor.clear()
            reach = max([last] + [j for (i, j) in m.__data if i < last])
            head = {k: v for k, v in m.__data.items() if k[0] <= reach and k[1] <= reach}
            tables.append(engine.BlockTable(np.ascontiguousarray(m.__row_index[:reach + 2], dtype=np.int32), head))
            inverses.append(m.__inverse_table()[:reach + 1])
        pivots = engine.block_potrf_pair(tables[0], inverses[0], tables[1], inverses[1], first, last)
        for m in (self, other):
            m._holds_factor_inverses = m._inverse_in_place
        for pivot in pivots:
            if pivot:
                raise np.linalg.LinAlgError('{0}-th leading minor of the array is not positive definite'.format(pivot))

    def _solve_rows(self, x, transpose, first, last):
        """in place on the device tensor x [n, k]: the sweep of solve_triangular over the block rows first <= r < last only
        (shg_block_solve_rows)"""
        engine.block_solve_rows(self.__block_table(), self.__inverse_table(), bool(transpose), first, last, x)
        return x

    def _sparse_inverse_rows(self, first, last):
        """sparse_inverse() for the block rows last - 1 .. first; the blocks of the later rows hold their entries of the inverse
        already (shg_block_sparse_inverse_rows).  The matrix is an ordinary (covariance) matrix afterwards."""
        engine.block_sparse_inverse_rows(self.__block_table(), self.__inverse_table(), first, last)
        self.__inverse_factor.clear()
        self._inverse_in_place = False
        self._holds_factor_inverses = False

    def __vector(self, b):
        v = _dev(b)
        return v.reshape(1, -1) if v.dim() == 1 else v

    def multiply_triangular(self, b, transpose=False):
        """v = W b or v = W^T b with the upper triangular factor (grates/lstsq.py:719-750).  As upstream, the transposed
        branch assigns instead of accumulating (lstsq.py:743)."""
        self.__require_plain_factor('multiply_triangular')
        bd = self.__vector(b)
        v = engine.block_multiply(self.__block_table(), 1 if transpose else 0, bd)
        return _like_input(v, b)

    def multiply_symmetric(self, b):
        """v = N b for a symmetric matrix of which only the upper triangle is stored (grates/lstsq.py:752-776)"""
        bd = self.__vector(b)
        return _like_input(engine.block_multiply(self.__block_table(), 2, bd), b)

    def solve_triangular(self, b, transpose=False):
        """Solve W x = b or W^T x = b with the upper triangular block factor (grates/lstsq.py:778-821)."""
        x = self.__vector(b)                                  # a copy: solved in place
        self.__ensure_factor_inverses()
        engine.block_solve(self.__block_table(), self.__inverse_table(), bool(transpose), x)
        return _like_input(x, b)

    def __ensure_factor_inverses(self):
        """inverses of the diagonal factor blocks that are not cached (a factor that was stored block by block rather than computed
        by cholesky(): grates/lstsq.py:807, 817 invert / solve with the diagonal blocks on the fly)"""
        for i in range(self.shape[0]):
            if i not in self.__inverse_factor:
                self.__inverse_factor[i] = self.__data[(i, i)] if self._holds_factor_inverses else engine.trtri(self.__data[(i, i)])

    def sparse_inverse(self):
        """
        Sparse inverse N^-1 = W^-1 W^-T on the pattern of the Cholesky factor W held by the matrix, in place
        (grates/lstsq.py:823-846).
        """
        self.__ensure_factor_inverses()
        engine.block_sparse_inverse(self.__block_table(), self.__inverse_table())
        self.__inverse_factor.clear()
        self._inverse_in_place = False
        self._holds_factor_inverses = False

    def inverse(self):
        """
        Full inverse N^-1 = W^-1 W^-T from the Cholesky factor W held by the matrix, in place, upper triangle
        (grates/lstsq.py:848-882).
        """
        self.__require_plain_factor('inverse')
        nb = self.shape[0]
        for i in range(nb):
            for j in range(i, nb):
                self.__set_block(i, j)                        # the inverse of a banded factor is dense
        self.__ensure_factor_inverses()
        engine.block_inverse(self.__block_table(), self.__inverse_table())
        self.__inverse_factor.clear()

    def _scale(self, value):
        """Scale whole matrix with a factor."""
        self.__require_plain_factor('_scale')
        for block in self.__data.values():
            engine.axpby(value, block, 0.0, block)
        self.__inverse_factor.clear()

    def _axpy(self, factor, other):
        """Perform self += factor * other."""
        self.__require_plain_factor('_axpy')
        other.__require_plain_factor('_axpy')
        for key, block in other.__data.items():
            if key in self.__data:
                engine.axpby(factor, block, 1.0, self.__data[key])
            else:
                self.__data[key] = _zeros(block.shape)
                engine.axpby(factor, block, 0.0, self.__data[key])
        self.__inverse_factor.clear()

    def diag(self):
        """Return copy of main diagonal."""
        d = np.zeros(min(self.__row_index[-1], self.__column_index[-1]))
        for idx in range(min(len(self.__row_index), len(self.__column_index)) - 1):
            if self.__nz(idx, idx):
                d[self.__row_index[idx]:self.__row_index[idx + 1]] = engine.to_host(self.__data[(idx, idx)].diagonal())
        return d


class NormalEquations:
    """Normal equations N x = n of a least-squares problem: block matrix N (upper blocks), right-hand side n [n, 1] (ndarray or
    device tensor), l^T P l and the number of observations (grates/lstsq.py:915-1059).  `status` tracks what `matrix` currently
    holds: 'normal_matrix', 'cholesky_factor' or 'covariance_matrix'."""

    def __init__(self, normal_matrix, right_hand_side, observation_square_sum, observation_count):
        self.matrix, self.right_hand_side = normal_matrix, right_hand_side
        self.observation_square_sum, self.observation_count = observation_square_sum, observation_count
        self.status = 'normal_matrix'

    DESIGN_BLOCK_BYTES = 256 << 20      # budget of one block of the transposed design matrix in from_accelerations
    arc_elimination = None              # ArcElimination of a system built under ArcParameters
    ARC_UPDATE_COLUMNS = 256            # columns of D that N -= D D^T waits for: the update reads and writes all of N, whatever its rank

    @classmethod
    def default_block_points(cls, parameters, components):
        """Default block of every from_* and of_* (3 components for accelerations, K for gradients, 1 for the line of sight, potentials
        and potential differences): the largest multiple of 256 points that keeps At [parameters, components Mb] within
        DESIGN_BLOCK_BYTES, at least 256."""
        return max(cls.DESIGN_BLOCK_BYTES // (8 * components * parameters) // 256 * 256, 256)

    @classmethod
    def _normals(cls, observations, model, block_points, windows=None):
        """Every from_* behind the checks of its observations (an _Observations) under a _StochasticModel.  Per block of _design_blocks
        N += At At^T, n += At l and l^T P l += |l|^2 on the fp64 MFMA product; both triangles of N are computed and the upper one is
        mirrored.  Under ArcParameters the parameters of the arcs are eliminated block by block (_ArcSetup, _ArcSweep), with
        l^T P l -= |R^T b|^2 and observation_count -= sum of the ranks.  windows (the _Windows of a TemporalParameters call; default
        None: nothing here changes) sends the call to _temporal_normals."""
        if windows is not None:
            return cls._temporal_normals(observations, model, block_points, windows)
        block_points = _prepare(observations, model, block_points)
        torch = engine.require_gpu()
        P = observations.P
        normals, side, square_sum = _zeros((P, P)), _zeros((P, 1)), _zeros((1, 1))
        sweep = _ArcSweep(observations, model, normals, side, cls.ARC_UPDATE_COLUMNS) if model.parameters is not None else None
        for first, last, At, lb, _, _ in _design_blocks(observations, model, block_points):
            engine.gemm(At, At, transb=True, beta=1.0, out=normals)
            engine.gemm(At, lb, beta=1.0, out=side)
            engine.gemm(lb, lb, transa=True, beta=1.0, out=square_sum)
            if sweep is not None:
                sweep.block(first, last, At)
        if sweep is not None:
            sweep.flush()
        _mirror_upper(normals)
        matrix = BlockMatrix([0, P], [0, P])
        matrix._set_device(0, 0, normals)
        system = cls(matrix, side, float(square_sum.item()), observations.K * observations.M)
        if sweep is not None:
            system.arc_elimination = sweep.result()
            system.observation_square_sum -= float(np.sum(sweep.setup.g * sweep.setup.g))
            system.observation_count -= system.arc_elimination.count
        return system

    @classmethod
    def _temporal_normals(cls, observations, model, block_points, windows):
        """The from_* of TemporalParameters: the normal matrix is block-banded in the B fields.  Per block of
        _temporal_design_blocks and pair of its slots a <= b whose supports intersect, block (f + a, f + b) += S~[a] S~[b]^T over the
        columns of the intersection alone, n[f + a] += S~[a] l~ and l^T P l += |l~|^2, all on the fp64 MFMA product.  Where the
        intersection is the whole block (always without a noise model) the product is the one call of _normals on At [P, K Mb];
        elsewhere one call per component, on column slices.  Both triangles of a diagonal block are computed and the upper one is
        mirrored, as _normals mirrors; a block (f, f') that no pair touches is not stored."""
        _prepare(observations, model, block_points, windows=windows)
        torch = engine.require_gpu()
        P, K, B = observations.P, observations.K, windows.B
        blocks, side, square_sum = {}, _zeros((B * P, 1)), _zeros((1, 1))
        for block, St, lb, _, _ in _temporal_design_blocks(observations, model, windows):
            points = block.last - block.first
            for a, support in enumerate(block.supports):
                if support is not None:
                    field = block.field + a
                    engine.gemm(St[a], lb, beta=1.0, out=side[field * P:(field + 1) * P])
            for a, b, c0, c1 in _slot_pairs(block):
                key = (block.field + a, block.field + b)
                if key not in blocks:
                    blocks[key] = _zeros((P, P))
                if (c0, c1) == (0, points):
                    engine.gemm(St[a], St[b], transb=True, beta=1.0, out=blocks[key])
                else:
                    left, right = St[a].reshape(P, K, points), St[b].reshape(P, K, points)
                    for k in range(K):
                        engine.gemm(left[:, k, c0:c1], right[:, k, c0:c1], transb=True, beta=1.0, out=blocks[key])
            engine.gemm(lb, lb, transa=True, beta=1.0, out=square_sum)
        block_index = np.arange(0, (B + 1) * P, P, dtype=int)
        matrix = BlockMatrix(block_index, block_index)
        for (row, column), block in sorted(blocks.items()):
            if row == column:
                _mirror_upper(block)
            matrix._set_device(row, column, block)
        return cls(matrix, side, float(square_sum.item()), observations.K * observations.M)

    @classmethod
    def from_accelerations(cls, xyz, g, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None, block_points=None,
                           noise_model=None, arcs=None):
        """
        Normal equations of the coefficients of degrees min_degree .. max_degree (in the order of utilities.ravel_coefficients) from
        accelerations g [M, 3] observed at the cartesian positions xyz [M, 3] (host arrays or device tensors; g is usually reduced by
        a reference field).  weights [M] per point or [M, 3] per component (finite, >= 0; default 1) are those of the observations.

        The points are taken in blocks of `block_points` (default: the largest multiple of 256 that keeps a block of the design
        matrix within 256 MB, at least 256).  Per block the transposed design matrix At [P, 3 Mb], scaled by sqrt(w), comes from
        shg_acceleration_design, and N += At At^T, n += At (sqrt(w) g) and l^T P l += |sqrt(w) g|^2 run on the fp64 MFMA product
        (both triangles of N are computed; the upper one is mirrored at the end, so that N is exactly symmetric).

        noise_model: coloured noise along the series of points.  One AutoregressiveModelSequence of dimension 1 (shared by the
        components) or a sequence of them, one per component, of maximum order q <= 128: every arc is decorrelated with the
        lower-triangular banded W, W^T W = Sigma^-1 = noise_model.normal_equations(arc length) (whitening_taps, shg_whiten_rows), applied
        to the design matrix and to the observations before the three products.  arcs holds the start indices of the arcs, ascending
        from 0 (default: one arc); nothing crosses an arc boundary, and every arc starts with the exact start-up (orders 0, 1, ...,
        q).  A data gap is a new arc, not a zero weight: a zero weight leaves the point in the filter's history.  Weights keep their
        meaning and scale the rows by sqrt(w) before the whitening, so the weight matrix in effect is D^1/2 W^T W D^1/2.  block_points
        keeps its default: a block takes up to q points in front of it along as history, the whitened copy doubles the peak memory of
        a block, and observation_count is unchanged.  noise_model=None changes nothing; arcs without it is a ValueError.
        A CovarianceFunction (or one per component) in place of the sequences gives every arc of up to q + 1 points its full
        covariance matrix, q <= 4095, and the AR(q) continuation beyond (shg_whiten_rows_long above q = 128).
        ColouredNoise(noise_model, arcs) offers the same for all five kinds of observation; ArcParameters(basis, arcs, noise_model)
        also eliminates parameters that last one arc (biases, drifts, once-per-revolution terms).

        Returns NormalEquations with a one-block BlockMatrix [P, P] and the right-hand side [P, 1] on the device, and
        observation_count = 3 M: components of zero weight still count as observations.
        """
        return _route('accelerations', dict(xyz=xyz, g=g, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), _StochasticModel(noise_model, arcs), block_points)

    @classmethod
    def from_gradients(cls, xyz, gradients, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, frames=None, components=None,
                       weights=None, block_points=None):
        """
        Normal equations of the coefficients of degrees min_degree .. max_degree (in the order of utilities.ravel_coefficients) from
        gravitational gradients observed at the cartesian positions xyz [M, 3] (host arrays or device tensors; usually reduced by a
        reference field).  frames [M, 3, 3] hold the instrument axes of every point as rows, in Earth-fixed coordinates (None: the
        observations are Earth-fixed); components is a sequence of distinct names from ('xx', 'xy', 'xz', 'yy', 'yz', 'zz') in any
        order (default: all six), K of them.  gradients is [M, K] in that canonical order, or [M, 3, 3], of which the selected
        upper-triangle entries are taken.  weights [M] per point or [M, K] per selected component (finite, >= 0; default 1).

        The block loop of from_accelerations with At [P, K Mb] from shg_gradient_design; the default block is the largest multiple of
        256 points that keeps At within 256 MB, at least 256.  Returns NormalEquations with a one-block BlockMatrix [P, P] and the
        right-hand side [P, 1] on the device, and observation_count = K M.

        Coloured noise: ColouredNoise(noise_model, arcs).from_gradients(the same arguments), with one scalar
        AutoregressiveModelSequence for all K selected components or one per component in canonical order (the gradiometer's coloured
        noise), every arc decorrelated on its own as in from_accelerations.  A data gap is a new arc, not a zero weight; block_points
        keeps its default, the peak memory of a block doubles and observation_count is unchanged.
        """
        return _route('gradients', dict(xyz=xyz, gradients=gradients, frames=frames, components=components, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), None, block_points)

    @classmethod
    def from_line_of_sight(cls, xyz_a, xyz_b, differences, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, directions=None,
                           weights=None, block_points=None):
        """
        Normal equations of the coefficients of degrees min_degree .. max_degree (in the order of utilities.ravel_coefficients) from
        line-of-sight gravity differences l_i = e_i . (g(b_i) - g(a_i)) [M] of M satellite pairs at the cartesian positions xyz_a
        [M, 3] and xyz_b [M, 3] (host arrays or device tensors; usually reduced by a reference field).  directions [M, 3] are the lines
        of sight e (unit vectors within 1e-12); without them e = (b - a) / |b - a|, and no pair may coincide.  weights [M] (finite,
        >= 0; default 1) are those of the observations.

        The block loop of from_accelerations with At [P, Mb] from shg_los_design; the default block is the largest multiple of 256
        pairs that keeps At within 256 MB, at least 256.  Returns NormalEquations with a one-block BlockMatrix [P, P] and the
        right-hand side [P, 1] on the device, and observation_count = M.  Normals of the same degrees add up through
        accumulate_normals, those of from_accelerations included: the combination of orbit and link.

        Coloured noise: ColouredNoise(noise_model, arcs).from_line_of_sight(the same arguments), with one scalar
        AutoregressiveModelSequence (the link's noise is correlated along the arc), every arc decorrelated on its own as in
        from_accelerations.  A data gap is a new arc, not a zero weight; block_points keeps its default, the peak memory of a block
        doubles and observation_count is unchanged.
        """
        return _route('line_of_sight', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, directions=directions, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), None, block_points)

    @classmethod
    def from_potentials(cls, xyz, potentials, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None, block_points=None):
        """
        Normal equations of the coefficients of degrees min_degree .. max_degree (in the order of utilities.ravel_coefficients) from
        the gravitational potential V [M] observed at the cartesian positions xyz [M, 3] (host arrays or device tensors; usually
        reduced by a reference field): the observation of the energy-balance approach, the kinetic energy of a satellite less the
        terms the caller has removed (the centrifugal potential and the dissipative integrals of the energy equation are the caller's
        reduction and no part of this).  weights [M] (finite, >= 0; default 1) are those of the observations.

        The energy integral leaves one unknown constant per arc: ArcParameters(arc_basis(arcs, M, degree=0), arcs).from_potentials(the
        same arguments) estimates and eliminates it; use min_degree >= 1 there, the constant of an arc and C_00 are hardly separable.
        ColouredNoise(noise_model, arcs).from_potentials decorrelates every arc with one scalar AutoregressiveModelSequence.

        The block loop of from_accelerations with At [P, Mb] from shg_potential_design; the default block is the largest multiple of
        256 points that keeps At within 256 MB, at least 256.  Returns NormalEquations with a one-block BlockMatrix [P, P] and the
        right-hand side [P, 1] on the device, and observation_count = M.  Normals of the same degrees add up through accumulate_normals.
        """
        return _route('potentials', dict(xyz=xyz, potentials=potentials, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), None, block_points)

    @classmethod
    def from_potential_differences(cls, xyz_a, xyz_b, differences, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None,
                                   block_points=None):
        """
        Normal equations of the coefficients of degrees min_degree .. max_degree (in the order of utilities.ravel_coefficients) from
        potential differences V(b_i) - V(a_i) [M] of M satellite pairs at the cartesian positions xyz_a [M, 3] and xyz_b [M, 3] (host
        arrays or device tensors; usually reduced by a reference field): the inter-satellite observation of the energy-balance approach,
        from the range-rate of the pair, with the caller's reductions as in from_potentials.  Pairs may coincide (a zero row).  weights
        [M] (finite, >= 0; default 1) are those of the observations.  ArcParameters and ColouredNoise bind it as they bind
        from_potentials.

        The block loop of from_accelerations with At [P, Mb] from shg_potential_difference_design; the default block as in
        from_potentials.  Returns NormalEquations with a one-block BlockMatrix [P, P] and the right-hand side [P, 1] on the device, and
        observation_count = M.
        """
        return _route('potential_differences', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), None, block_points)

    def __cholesky(self):
        """factor the matrix once; a matrix that already holds covariances cannot be factored again (ValueError, as upstream)"""
        if self.status == 'covariance_matrix' or self.status not in ('normal_matrix', 'cholesky_factor'):
            raise ValueError('the matrix holds {0}: only a normal matrix can be factored'.format(self.status))
        if self.status == 'normal_matrix':
            self.matrix.cholesky()
            self.status = 'cholesky_factor'

    def solve(self, signs=None):
        """
        Solve the system; the coefficient matrix afterwards holds the upper triangular Cholesky factor.  As upstream, 100
        Monte-Carlo vectors of random signs (numpy.random.randint, global state, drawn on the host so that a seeded run
        reproduces the reference) are solved along with the right-hand side and kept in `monte_carlo_vectors`
        (grates/lstsq.py:950-968).

        signs : ndarray or device tensor [n, k] of +-1, optional (extension)
            Monte-Carlo vectors to use instead of the host draw (5e8 draws and a 5 GB upload for config 5).
        """
        self.__cholesky()
        rhs = _dev(self.right_hand_side)
        h = self.matrix.solve_triangular(rhs, transpose=True)
        if signs is None:
            xi = np.random.randint(0, 2, size=(h.shape[0], 100))
            xi[xi == 0] = -1
            signs = xi.astype(np.float64)
        torch = engine.require_gpu()
        x = self.matrix.solve_triangular(torch.cat((h, _dev(signs)), dim=1))
        if _is_tensor(self.right_hand_side):
            self.monte_carlo_vectors = x[:, 1:]
            return x[:, 0:1]
        x = engine.to_host(x)
        self.monte_carlo_vectors = x[:, 1:]
        return x[:, 0:1]

    def redundancy(self, combined_normals, variance_factor):
        """grates/lstsq.py:970-988"""
        mc = _dev(combined_normals.monte_carlo_vectors)
        Nm = self.matrix.multiply_symmetric(mc)
        estimated_trace = _dot(mc, Nm) / mc.shape[1]
        return np.asarray(self.observation_count - estimated_trace / variance_factor).squeeze()

    def residual_square_sum(self, solution):
        """grates/lstsq.py:990-1005"""
        x = _dev(solution)
        Nx = self.matrix.multiply_symmetric(x)
        rhs = _dev(self.right_hand_side)
        return np.asarray(self.observation_square_sum - 2 * _dot(rhs, x) + _dot(x, Nx)).squeeze()

    def posterior_sigma(self, solution):
        """grates/lstsq.py:1007-1024"""
        x = _dev(solution)
        Wx = self.matrix.multiply_triangular(x)
        rhs = _dev(self.right_hand_side)
        ePe = self.observation_square_sum - 2 * _dot(rhs, x) + _dot(Wx, Wx)
        return np.sqrt(ePe / (self.observation_count - x.shape[0])).squeeze()

    def compute_covariance(self, sparse=True):
        """(sparse) inverse of the coefficient matrix (grates/lstsq.py:1026-1042)"""
        self.__cholesky()
        (self.matrix.sparse_inverse if sparse else self.matrix.inverse)()
        self.status = 'covariance_matrix'

    def to_array(self):
        """grates/lstsq.py:1044-1059"""
        rhs = engine.to_host(self.right_hand_side) if _is_tensor(self.right_hand_side) else self.right_hand_side
        return self.matrix.to_array(), rhs, self.observation_square_sum, self.observation_count


class TikhonovRegularization(NormalEquations):
    """Normal equations of a Tikhonov regularization with a diagonal regularization matrix (grates/lstsq.py:1062-1088)."""

    def __init__(self, regularization_vector, block_index, right_hand_side=None):
        weights = np.asarray(regularization_vector)
        if right_hand_side is None:                            # zero bias: zero right-hand side, l^T P l = 0
            bias, weighted_square_sum = np.zeros((block_index[-1], 1)), 0
        else:                                                  # bias b with weights w: n = w * b, l^T P l = sum(w b^2)
            weighted_square_sum = np.sum(right_hand_side**2 * weights[:, np.newaxis])
            bias = right_hand_side * weights[:, np.newaxis]
        diagonal = BlockMatrix(block_index, block_index)
        for k, (lo, hi) in enumerate(zip(block_index[:-1], block_index[1:])):
            diagonal[k, k] = np.diag(weights[lo:hi])
        super().__init__(diagonal, bias, weighted_square_sum, bias.size)


class _BoundModel:
    """the from_* of ColouredNoise and ArcParameters, one per kind of observation: the arguments of the classmethods of NormalEquations,
    the normals under this model"""

    def from_accelerations(self, xyz, g, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None, block_points=None):
        return _route('accelerations', dict(xyz=xyz, g=g, weights=weights), engine.Band(min_degree, max_degree, GM, R), self, block_points)

    def from_gradients(self, xyz, gradients, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, frames=None, components=None,
                       weights=None, block_points=None):
        return _route('gradients', dict(xyz=xyz, gradients=gradients, frames=frames, components=components, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self, block_points)

    def from_line_of_sight(self, xyz_a, xyz_b, differences, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, directions=None,
                           weights=None, block_points=None):
        return _route('line_of_sight', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, directions=directions, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self, block_points)

    def from_potentials(self, xyz, potentials, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None, block_points=None):
        return _route('potentials', dict(xyz=xyz, potentials=potentials, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self, block_points)

    def from_potential_differences(self, xyz_a, xyz_b, differences, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None,
                                   block_points=None):
        return _route('potential_differences', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self, block_points)


class ColouredNoise(_BoundModel):
    """
    A noise model of the observations along the series of points, bound to the constructors of NormalEquations: noise_model is one
    scalar AutoregressiveModelSequence or CovarianceFunction (shared by the components) or a sequence of them, one per component, arcs
    the start indices of the arcs (default: one arc), as NormalEquations.from_accelerations describes them.  from_accelerations, from_gradients,
    from_line_of_sight, from_potentials and from_potential_differences take the arguments of the classmethods of the same name and
    return the NormalEquations of the decorrelated observations.  The model is checked here (whitening_taps), the arcs against the number of points in every call; all of it before
    anything reaches the device.  A VectorNoise in place of the scalar models whitens the K components of a point jointly; its
    dimension must be the K of the observations of every call.
    """

    def __init__(self, noise_model, arcs=None):
        _WhiteningTables(noise_model)
        self.noise_model, self.arcs = noise_model, arcs


class ArcParameters(_BoundModel):
    """
    Parameters that last one arc (an accelerometer's bias and drift per axis, a gradiometer's bias per component, the link's empirical
    once-per-revolution terms), estimated per arc and eliminated from the normal equations before the arcs are summed; bound to the
    constructors of NormalEquations like ColouredNoise.  basis is [M, u'] (shared: every component of every arc has u' parameters of
    its own, whose design matrix is the basis on the points of the arc; arc_basis) or [M, K, u] (general: every arc has one set of u
    parameters, of which component k of point t sees basis[t, k, :]; frame_basis), u and u' at most 16.  arcs holds the start
    indices of the arcs (default: one arc); noise_model is that of ColouredNoise, with the same arcs.  The basis goes the way of
    the design matrix: times sqrt(w), then the arc's W.

    from_accelerations, from_gradients, from_line_of_sight, from_potentials and from_potential_differences take the arguments of the
    classmethods of the same name and return the NormalEquations of the coefficients alone, N = A^T A - sum_a C_a G_a^+ C_a^T with C_a = A_a^T B_a, G_a = B_a^T B_a (n and l^T P l
    alike), with observation_count reduced by the sum of the ranks of the G_a: posterior_sigma, redundancy and
    compute_variance_factors see the redundancy of the eliminated system.  Directions of G_a with eigenvalues at or below 1e-12 of the
    largest are dropped (an arc shorter than u', an arc of zero weights).  ne.arc_elimination (ArcElimination) holds the ranks and,
    with keep=True, returns the parameters of a solution; it then retains P K u' doubles per arc on the device (shared basis; P u
    for the general form).  The shape of the basis is checked against the points and components of every call, all of it before
    anything reaches the device.
    """

    def __init__(self, basis, arcs=None, noise_model=None, keep=True):
        basis = np.asarray(engine.to_host(basis) if _is_tensor(basis) else basis, dtype=np.float64)
        if basis.ndim not in (2, 3):
            raise ValueError('the arc basis must have shape (M, u) or (M, K, u), got {0}'.format(basis.shape))
        if not 1 <= basis.shape[-1] <= MAX_ARC_PARAMETERS:
            raise ValueError('{0} parameters per arc: expected 1 .. {1}'.format(basis.shape[-1], MAX_ARC_PARAMETERS))
        if not np.all(np.isfinite(basis)):
            raise ValueError('the arc basis must be finite')
        if noise_model is not None:
            _WhiteningTables(noise_model)
        if isinstance(noise_model, VectorNoise) and basis.ndim == 2:
            raise ValueError('a shared arc basis (M, u) gives every component parameters of its own, which a VectorNoise couples: pass the '
                             'general basis lstsq.component_basis(basis, {0}) of shape (M, {0}, {0} u)'.format(noise_model.dimension))
        self.basis, self.arcs, self.noise_model, self.keep = basis, arcs, noise_model, bool(keep)


class RadialBasisParameters:
    """
    The node values of an isotropic gravityfield.RadialBasisFunctions as the parameters of a least-squares problem, bound to the
    constructors of NormalEquations and of PostFit like ColouredNoise and ArcParameters: a regional solution (a basin, an ice sheet,
    mascon-like nodes) from the observations the spherical harmonic route takes.  basis gives the nodal points, the shape factors
    (degree_factors: ValueError for an anisotropic K), the band min_degree .. max_degree, GM and R, so the calls take none of them;
    model is None (white noise), a ColouredNoise or an ArcParameters, as PostFit takes it.

    from_accelerations, from_gradients, from_line_of_sight, from_potentials and from_potential_differences take the observations,
    weights and block_points of the classmethods of the same name (from_gradients also frames and components) and return
    NormalEquations [J, J] of the J node values: the block loop of NormalEquations.from_accelerations with At [J, K Mb] from
    shg_rbf_design or, for the gradient tensor, shg_rbf_gradient_design (a closed Legendre sum per point and node; neither the
    spherical harmonic design matrix nor to_potential_coefficients_matrix is formed), whitening, arc elimination and the products
    unchanged; the default block is default_block_points(J, K).  ``basis.values = engine.to_host(ne.solve())[:, 0]`` and
    ``basis.to_grid(...)`` close the chain.  of_accelerations ... of_potential_differences take the solution [J] first and vectors
    [J, S] last and return the PostFit of that solution under the model.  Every check runs before anything reaches the device.
    """

    def __init__(self, basis, model=None):
        _StochasticModel.of(model)
        basis.degree_factors
        self.basis, self.model = basis, model

    def from_accelerations(self, xyz, g, weights=None, block_points=None):
        return _route('accelerations', dict(xyz=xyz, g=g, weights=weights), engine.basis_band(self.basis), self.model, block_points)

    def from_gradients(self, xyz, gradients, frames=None, components=None, weights=None, block_points=None):
        return _route('gradients', dict(xyz=xyz, gradients=gradients, frames=frames, components=components, weights=weights),
                      engine.basis_band(self.basis), self.model, block_points)

    def from_line_of_sight(self, xyz_a, xyz_b, differences, directions=None, weights=None, block_points=None):
        return _route('line_of_sight', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, directions=directions, weights=weights),
                      engine.basis_band(self.basis), self.model, block_points)

    def from_potentials(self, xyz, potentials, weights=None, block_points=None):
        return _route('potentials', dict(xyz=xyz, potentials=potentials, weights=weights), engine.basis_band(self.basis), self.model, block_points)

    def from_potential_differences(self, xyz_a, xyz_b, differences, weights=None, block_points=None):
        return _route('potential_differences', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, weights=weights),
                      engine.basis_band(self.basis), self.model, block_points)

    def of_accelerations(self, solution, xyz, g, weights=None, block_points=None, vectors=None):
        return _route('accelerations', dict(xyz=xyz, g=g, weights=weights),
                      engine.basis_band(self.basis), self.model, block_points, fit=PostFit(solution, vectors, self.model, xyz))

    def of_gradients(self, solution, xyz, gradients, frames=None, components=None, weights=None, block_points=None, vectors=None):
        return _route('gradients', dict(xyz=xyz, gradients=gradients, frames=frames, components=components, weights=weights),
                      engine.basis_band(self.basis), self.model, block_points, fit=PostFit(solution, vectors, self.model, xyz))

    def of_line_of_sight(self, solution, xyz_a, xyz_b, differences, directions=None, weights=None, block_points=None, vectors=None):
        return _route('line_of_sight', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, directions=directions, weights=weights),
                      engine.basis_band(self.basis), self.model, block_points, fit=PostFit(solution, vectors, self.model, xyz_a))

    def of_potentials(self, solution, xyz, potentials, weights=None, block_points=None, vectors=None):
        return _route('potentials', dict(xyz=xyz, potentials=potentials, weights=weights),
                      engine.basis_band(self.basis), self.model, block_points, fit=PostFit(solution, vectors, self.model, xyz))

    def of_potential_differences(self, solution, xyz_a, xyz_b, differences, weights=None, block_points=None, vectors=None):
        return _route('potential_differences', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, weights=weights),
                      engine.basis_band(self.basis), self.model, block_points, fit=PostFit(solution, vectors, self.model, xyz_a))


def _check_windows(first, factors, fields):
    """(first [M] int64, factors [M, W] float64, B) of a window model, on the host: factors [M, W] finite, 1 <= W <= 16, first [M] integers
    with 0 <= first <= B - W, B = fields an integer; ValueError otherwise"""
    if _is_tensor(factors):
        factors = engine.to_host(factors)
    factors = np.asarray(factors, dtype=np.float64)
    if factors.ndim != 2:
        raise ValueError('factors must have shape (M, W), got {0}'.format(factors.shape))
    M, W = factors.shape
    if not 1 <= W <= MAX_TEMPORAL_SLOTS:
        raise ValueError('a window of {0} fields: expected 1 .. {1}'.format(W, MAX_TEMPORAL_SLOTS))
    first = np.asarray(first)
    if first.shape != (M,) or first.dtype.kind not in 'iu':
        raise ValueError('first must be an integer array of shape ({0},), got {1} of {2}'.format(M, first.dtype, first.shape))
    first = first.astype(np.int64)
    if isinstance(fields, bool) or int(fields) != fields:
        raise ValueError('fields must be an integer, got {0!r}'.format(fields))
    B = int(fields)
    if B < W:
        raise ValueError('a window of {0} fields, but only {1} fields'.format(W, B))
    if M and (int(first.min()) < 0 or int(first.max()) > B - W):
        bad = int(np.flatnonzero((first < 0) | (first > B - W))[0])
        raise ValueError('first[{0}] is {1}, outside 0 .. {2} ({3} fields, windows of {4})'.format(bad, int(first[bad]), B - W, B, W))
    if not np.all(np.isfinite(factors)):
        raise ValueError('factors must be finite')
    return first, np.ascontiguousarray(factors), B


def _take(values, order):
    """the entries `order` of a per-point argument (None, a host array or a device tensor) along its first axis"""
    if values is None:
        return None
    if _is_tensor(values):
        return values.index_select(0, engine._torch().from_numpy(order).to(values.device))
    return np.asarray(values)[order]


class _Windows:
    """The window model of one from_* or of_* call under a TemporalParameters, for M points: first and factors in the order the call
    works in, W, B and `order`, the stable sort by `first` that a call without a noise model applies where first decreases somewhere
    (None otherwise; it is applied to the per-point arguments of the observations here, before their upload, and restore() puts the last
    axis of a result back).  plan() fills blocks (temporal_blocks) on the host, to_device() the factors on the device."""

    def __init__(self, temporal, observations):
        if temporal.first.shape[0] != observations.M:
            raise ValueError('{0} points but the temporal parameters hold the windows of {1}'.format(observations.M, temporal.first.shape[0]))
        self.first, self.factors, self.B, self.W = temporal.first, temporal.factors, temporal.field_count, int(temporal.factors.shape[1])
        self.order = None if temporal.model is not None else engine.points_at_plan(self.first)[0]
        if self.order is not None:
            self.first, self.factors = self.first[self.order], np.ascontiguousarray(self.factors[self.order])
            observations.take(self.order)
        self.blocks = self.device_factors = None

    def restore(self, sorted_values):
        torch = engine._torch()
        index = torch.from_numpy(self.order).to(sorted_values.device)
        return torch.empty_like(sorted_values).index_copy_(sorted_values.dim() - 1, index, sorted_values)

    def default_block_points(self, parameters, components):
        return TemporalParameters.default_block_points(parameters, components, self.W)

    def plan(self, model, block_points):
        self.blocks = temporal_blocks(self.first, self.W, block_points, None if model.whitening is None else model.whitening.stage)

    def to_device(self, device):
        self.device_factors = engine.to_device(self.factors, device)


def _as_mjd(epochs):
    from . import utilities
    return epochs if isinstance(epochs, np.ndarray) else np.array([utilities._mjd(epoch) for epoch in epochs], dtype=np.float64)


class TemporalParameters:
    """
    Parameters that vary in time, bound to the constructors of NormalEquations and of PostFit like ColouredNoise, ArcParameters and
    RadialBasisParameters: B = `fields` sets of the P coefficients of degrees min_degree .. max_degree, of
    which point i sees the W consecutive ones first[i] .. first[i] + W - 1 with the factors[i, :] -- the window model of the *_at
    functionals (gravityfield._FunctionalsAtEpochs), read backwards.  The design row of an observation of point i with respect to field
    f is factors[i, f - first[i]] times its static row (gravityfield.temporal_design_matrix states that for small M), so the normal
    matrix is block-banded in the fields.  The parameter vector is field-major, x = [x_0 .. x_(B-1)], each x_f [P] in the order of
    utilities.ravel_coefficients; fields(x) returns it as [B, P].

    first [M] host ints, 0 <= first <= B - W; factors [M, W] finite and signed, 1 <= W <= 16; model None (white noise) or a
    ColouredNoise.  An ArcParameters is a ValueError: arc elimination under temporal parameters is not built yet.  linear (nodes in
    time with linear interpolation, W = 2), constant (independent fields per interval, W = 1) and harmonic (static part, trend and
    cycles, one window of all fields) compute first and factors on the host, in float64.  Every check runs before anything reaches the
    device.

    from_accelerations, from_gradients, from_line_of_sight, from_potentials and from_potential_differences take the arguments of the
    classmethods of NormalEquations of the same name and return NormalEquations of the B P parameters: a BlockMatrix with block_index
    arange(0, (B + 1) P, P) that holds the upper blocks the observations touch (exactly symmetric diagonal blocks), the right-hand
    side [B P, 1] on the device and observation_count = K M.  accumulate_normals adds a process-dynamics constraint,
    AutoregressiveModelSequence.normal_equations(B) of dimension P; solve, compute_covariance, posterior_sigma, redundancy and
    compute_variance_factors work as on any block-banded system.  of_accelerations ... of_potential_differences take the solution [B P]
    or [B P, 1] first and vectors [B P, S] last and return the PostFit of that solution.

    Per block of points the transposed design matrix T [P, K, n] is expanded to the E <= 16 fields the block spans, S [E, P, K, n]
    (shg_window_expand), then whitened, then multiplied slot pair by slot pair.  Without a noise model points whose window starts
    decrease somewhere are sorted by them first (the normals are permutation-invariant; PostFit returns the residuals in the order
    given), blocks restart at every change of the window start and E = W.  With a noise model the order of the points is the order
    in time and is kept, and a block spans the window starts of its points and of the up to q points of history in front.
    block_points defaults to default_block_points(P, K, W).  Peak memory of a block of Mb points with history h in E slots:
    (1 + E) P K (Mb + h) doubles for T and S, and E P K Mb more for the whitened copy under a noise model.
    """

    def __init__(self, first, factors, fields, model=None):
        if isinstance(model, ArcParameters):
            raise ValueError('arc elimination under temporal parameters is not built yet: model must be None or a ColouredNoise')
        _StochasticModel.of(model)
        self.first, self.factors, self.field_count = _check_windows(first, factors, fields)
        self.model = model

    @staticmethod
    def default_block_points(parameters, components, window):
        """The default block of the from_* and of_* calls: the largest multiple of 256 points that keeps the expanded block
        S [W, parameters, components Mb] within NormalEquations.DESIGN_BLOCK_BYTES, at least 256."""
        return max(NormalEquations.DESIGN_BLOCK_BYTES // (8 * components * parameters * window) // 256 * 256, 256)

    @classmethod
    def linear(cls, nodes, epochs, model=None):
        """B = len(nodes) >= 2 fields at the ascending `nodes` in time, linear interpolation between them (W = 2): first and factors by
        the rule of TimeSeries.interpolation_windows (gravityfield.linear_interpolation_windows), bit for bit.  nodes and epochs [M] are
        each a sequence of datetime.datetime or a float64 array of modified Julian dates.  ValueError for nodes that do not ascend
        strictly and for an epoch outside them (no extrapolation)."""
        from .gravityfield import _check_epochs, linear_interpolation_windows
        nodes, epochs = _check_epochs(nodes, len(nodes)), _check_epochs(epochs, len(epochs))
        if any(not earlier < later for earlier, later in zip(nodes[:-1], nodes[1:])):
            raise ValueError('nodes must ascend strictly')
        first, factors = linear_interpolation_windows(nodes, epochs)
        return cls(first, factors, len(nodes), model)

    @classmethod
    def constant(cls, edges, epochs, model=None):
        """B = len(edges) - 1 independent fields, field k for the epochs of the half-open interval [e_k, e_(k+1)) (W = 1, factor 1.0):
        many solutions in one pass, block-diagonal normals.  edges and epochs [M] as in linear.  ValueError for fewer than two edges,
        edges that do not ascend strictly and an epoch outside them, naming the first one."""
        import bisect
        from .gravityfield import _check_epochs
        edges, epochs = _check_epochs(edges, len(edges)), _check_epochs(epochs, len(epochs))
        B = len(edges) - 1
        if B < 1 or any(not earlier < later for earlier, later in zip(edges[:-1], edges[1:])):
            raise ValueError('edges must be at least two and ascend strictly')
        if isinstance(edges, np.ndarray) or isinstance(epochs, np.ndarray):
            limits, values = _as_mjd(edges), _as_mjd(epochs)
            index = np.searchsorted(limits, values, side='right').astype(np.int64) - 1
        else:
            index = np.array([bisect.bisect_right(edges, epoch) - 1 for epoch in epochs], dtype=np.int64)
        outside = (index < 0) | (index >= B)
        if outside.any():
            k = int(np.flatnonzero(outside)[0])
            if isinstance(edges, np.ndarray) or isinstance(epochs, np.ndarray):
                raise ValueError('epoch {0} (MJD {1!r}) lies outside the edges ({2!r} .. {3!r}): the intervals are half-open'.format(
                    k, float(values[k]), float(limits[0]), float(limits[-1])))
            raise ValueError('epoch {0} ({1}) lies outside the edges ({2} .. {3}): the intervals are half-open'.format(k, epochs[k], edges[0], edges[-1]))
        return cls(index, np.ones((len(epochs), 1)), B, model)

    @classmethod
    def harmonic(cls, epochs, reference_epoch, periods=(), trend=True, static=True, time_scale=365.25, model=None):
        """One window of all B = W fields (first = 0): the static field (factor 1) if `static`, the trend per `time_scale` days (factor
        tau) if `trend`, then a cosine and a sine field per period [days] (factors cos and sin of 2 pi tau_T), tau the time since
        reference_epoch in units of time_scale and tau_T in units of the period -- the expressions, and the bits, of Trend.weights_at and
        Oscillation.weights_at (timevariable.epoch_arguments).  epochs [M] as in linear.  ValueError for a period or time_scale that is
        not finite and positive, and for no column at all or more than 16."""
        import datetime
        from .gravityfield import _check_epochs
        from .timevariable import Oscillation, Trend, epoch_arguments
        epochs = _check_epochs(epochs, len(epochs))
        if not isinstance(reference_epoch, datetime.datetime):
            raise ValueError('reference_epoch must be a datetime.datetime, got {0!r}'.format(reference_epoch))
        periods = np.asarray(periods, dtype=np.float64).reshape(-1)
        if not np.all(np.isfinite(periods) & (periods > 0)) or not (np.isfinite(time_scale) and time_scale > 0):
            raise ValueError('periods and time_scale must be finite and positive')
        columns = [np.ones((len(epochs), 1))] if static else []
        if trend:
            columns.append(Trend._weights_at(epoch_arguments(epochs, reference_epoch, 86400.0 * time_scale)))
        for period in periods:
            columns.append(Oscillation._weights_at(epoch_arguments(epochs, reference_epoch, 86400.0 * period)))
        if not columns:
            raise ValueError('no column at all: static, trend or a period is needed')
        factors = np.concatenate(columns, axis=1)
        return cls(np.zeros(len(epochs), dtype=np.int64), factors, factors.shape[1], model)

    def fields(self, x):
        """the solution x [B P] or [B P, 1] (host array or device tensor) as [B, P]"""
        size = int(np.prod(tuple(x.shape)))
        if len(x.shape) not in (1, 2) or (len(x.shape) == 2 and x.shape[1] != 1) or size % self.field_count:
            raise ValueError('the solution must have shape (B P,) or (B P, 1) with B = {0}, got {1}'.format(self.field_count, tuple(x.shape)))
        return x.reshape(self.field_count, size // self.field_count)

    def from_accelerations(self, xyz, g, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None, block_points=None):
        return _route('accelerations', dict(xyz=xyz, g=g, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self.model, block_points, self)

    def from_gradients(self, xyz, gradients, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, frames=None, components=None,
                       weights=None, block_points=None):
        return _route('gradients', dict(xyz=xyz, gradients=gradients, frames=frames, components=components, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self.model, block_points, self)

    def from_line_of_sight(self, xyz_a, xyz_b, differences, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, directions=None,
                           weights=None, block_points=None):
        return _route('line_of_sight', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, directions=directions, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self.model, block_points, self)

    def from_potentials(self, xyz, potentials, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None, block_points=None):
        return _route('potentials', dict(xyz=xyz, potentials=potentials, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self.model, block_points, self)

    def from_potential_differences(self, xyz_a, xyz_b, differences, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None,
                                   block_points=None):
        return _route('potential_differences', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self.model, block_points, self)

    def of_accelerations(self, solution, xyz, g, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None, block_points=None,
                         vectors=None):
        return _route('accelerations', dict(xyz=xyz, g=g, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self.model, block_points, self, PostFit(solution, vectors, self.model, xyz))

    def of_gradients(self, solution, xyz, gradients, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, frames=None, components=None,
                     weights=None, block_points=None, vectors=None):
        return _route('gradients', dict(xyz=xyz, gradients=gradients, frames=frames, components=components, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self.model, block_points, self, PostFit(solution, vectors, self.model, xyz))

    def of_line_of_sight(self, solution, xyz_a, xyz_b, differences, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, directions=None,
                         weights=None, block_points=None, vectors=None):
        return _route('line_of_sight', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, directions=directions, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self.model, block_points, self, PostFit(solution, vectors, self.model, xyz_a))

    def of_potentials(self, solution, xyz, potentials, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None,
                      block_points=None, vectors=None):
        return _route('potentials', dict(xyz=xyz, potentials=potentials, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self.model, block_points, self, PostFit(solution, vectors, self.model, xyz))

    def of_potential_differences(self, solution, xyz_a, xyz_b, differences, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06,
                                 weights=None, block_points=None, vectors=None):
        return _route('potential_differences', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), self.model, block_points, self, PostFit(solution, vectors, self.model, xyz_a))


class PostFit:
    """
    What a solution says about the stochastic model it was computed under: the residuals of the observations, the square sum, the
    redundancy and the variance factor of every arc, and the empirical covariance function of the residuals, from one more pass over
    the blocks of the design matrix.  of_accelerations, of_gradients, of_line_of_sight, of_potentials and
    of_potential_differences take the solution [P] or [P, 1] (host or device), then the arguments of the from_* of NormalEquations for
    the same kind with the same checks, then

    model   : None (white noise), the ColouredNoise or the ArcParameters the system was built with,
    vectors : [P, S], optional: the Monte-Carlo vectors of the solved (combined) system, ne.monte_carlo_vectors.

    Per block the whitened transposed design matrix At~ [P, K Mb] gives V = [x, z_1 .. z_S]^T At~ in one product on the fp64 MFMA
    GEMM, and a thin product on the unwhitened block the unwhitened model values.  The rows are kept whole on the device, `rows`
    [1 + S, K, M] doubles (row 0 is e~, row 1 + j the projected whitened model values of z_j): 1.3 GB for S = 100, K = 3, M = 5e5;
    pass the vectors in groups, or drop the attribute, if that is too much.
    Under ArcParameters the parameters of an arc are y^_a = R_a R_a^T B~_a^T (l~_a - A~_a x) with R_a as the elimination forms it, and
    every row v of V is projected explicitly, v - B~ R R^T (B~^T v), before it is squared (shg_segment_products for the basis products,
    shg_segment_lag_products at lags = 0 for all square sums).

    whitened [M, K]         e~ = l~ - A~ x - B~ y^; its square sum is ne.residual_square_sum(x) of the system of the same arguments
    residuals [M, K]        e^ = sqrt(w) (l - A x - B y^), not whitened: e~ = W e^
    arc_parameters          y^ [arcs, K, u'] (shared basis) or [arcs, u] (general form), host, zero along dropped directions; None
                            without ArcParameters.  ne.arc_elimination.parameters(x) without the kept columns: works after keep=False
    arcs, ranks             start indices [arcs]; ranks as ArcElimination.ranks (zeros [arcs, K] without ArcParameters)
    arc_observation_counts  n_a = K len_a - sum of the ranks of arc a
    arc_square_sums [arcs]  Omega_a = sum over the components and points of the arc of e~^2 (host)

    whitened and residuals are device tensors where the positions were, host arrays otherwise.  Without a model, and with
    ColouredNoise(arcs=None), there is the one arc [0].
    """

    def __init__(self, solution, vectors, model, template):
        _StochasticModel.of(model)
        self.__solution, self.__vectors, self.__template = solution, vectors, template
        self.__bound = self.__hat = None

    def _bind(self, observations, model, block_points, setup, temporal):
        """what leverages() runs the design blocks once more with: the _Observations, the _StochasticModel and block_points of the pass,
        under ArcParameters its _ArcSetup -- per-point tensors, small beside `rows`; temporal: the pass was one of TemporalParameters"""
        self.__bound, self.__hat = (observations, model, block_points, setup, bool(temporal)), None

    @classmethod
    def of_accelerations(cls, solution, xyz, g, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None, block_points=None,
                         model=None, vectors=None):
        return _route('accelerations', dict(xyz=xyz, g=g, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), model, block_points, fit=cls(solution, vectors, model, xyz))

    @classmethod
    def of_gradients(cls, solution, xyz, gradients, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, frames=None, components=None,
                     weights=None, block_points=None, model=None, vectors=None):
        return _route('gradients', dict(xyz=xyz, gradients=gradients, frames=frames, components=components, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), model, block_points, fit=cls(solution, vectors, model, xyz))

    @classmethod
    def of_line_of_sight(cls, solution, xyz_a, xyz_b, differences, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, directions=None,
                         weights=None, block_points=None, model=None, vectors=None):
        return _route('line_of_sight', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, directions=directions, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), model, block_points, fit=cls(solution, vectors, model, xyz_a))

    @classmethod
    def of_potentials(cls, solution, xyz, potentials, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06, weights=None, block_points=None,
                      model=None, vectors=None):
        return _route('potentials', dict(xyz=xyz, potentials=potentials, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), model, block_points, fit=cls(solution, vectors, model, xyz))

    @classmethod
    def of_potential_differences(cls, solution, xyz_a, xyz_b, differences, min_degree, max_degree, GM=3.9860044150e+14, R=6.3781363000e+06,
                                 weights=None, block_points=None, model=None, vectors=None):
        return _route('potential_differences', dict(xyz_a=xyz_a, xyz_b=xyz_b, differences=differences, weights=weights),
                      engine.Band(min_degree, max_degree, GM, R), model, block_points, fit=cls(solution, vectors, model, xyz_a))

    def _check(self, parameters):
        """the solution and the vectors against the number of parameters: ValueError before anything reaches the device"""
        shape = tuple(int(size) for size in np.shape(self.__solution))
        if shape not in ((parameters,), (parameters, 1)):
            raise ValueError('solution must have shape ({0},) or ({0}, 1), got {1}'.format(parameters, shape))
        if self.__vectors is not None:
            shape = tuple(int(size) for size in np.shape(self.__vectors))
            if len(shape) != 2 or shape[0] != parameters or shape[1] < 1:
                raise ValueError('vectors must have shape ({0}, S), got {1}'.format(parameters, shape))

    def _pass(self, observations, model, block_points, windows=None):
        """the pass over the blocks of NormalEquations._normals, with its arguments; returns self.  Under TemporalParameters (windows)
        the solution holds B fields, a block multiplies the columns of its own fields with its expanded design matrix, and points that
        the call sorted come back in the order they were given in"""
        block_points = _prepare(observations, model, block_points, self, windows)
        torch = engine.require_gpu()
        l, M, K, P = observations.l, observations.M, observations.K, observations.P
        parameters = P if windows is None else windows.B * P
        x = engine.to_device(self.__solution, l.device).reshape(parameters, 1)
        X = x if self.__vectors is None else torch.cat((x, engine.to_device(self.__vectors, l.device)), dim=1)
        rows = int(X.shape[1])
        Xt = torch.empty((rows, parameters), dtype=torch.float64, device=l.device).copy_(X.t())          # [1 + S, P], row stride P also for one row
        bounds = np.append(model.starts, M)
        arcs = len(bounds) - 1
        V = torch.empty((rows, K, M), dtype=torch.float64, device=l.device)                             # the whitened model values of x and the z_j
        lt, plain = torch.empty((K, M), dtype=torch.float64, device=l.device), torch.empty((K, M), dtype=torch.float64, device=l.device)
        blocks = _design_blocks(observations, model, block_points) if windows is None else _temporal_pass_blocks(observations, model, windows)
        for first, last, At, lb, At_plain, skip, *columns in blocks:
            Xb = Xt[:, columns[0]] if columns else Xt                                                    # the fields of the block
            V[:, :, first:last] = engine.gemm(Xb, At).reshape(rows, K, last - first)
            lt[:, first:last] = lb.reshape(K, last - first)
            if model.whitening is None:
                plain[:, first:last] = V[0, :, first:last]                                               # white noise: the same values
            else:
                plain[:, first:last] = engine.gemm(Xb[0:1], At_plain).reshape(K, skip + last - first)[:, skip:]
        V[0] = lt - V[0]                                                                                 # l~ - A~ x
        plain = l.t().contiguous() - plain                                                               # sqrt(w) (l - A x), dense [K, M]
        if windows is not None and windows.order is not None:
            V, plain = windows.restore(V), windows.restore(plain)
        seg = torch.from_numpy(bounds.astype(np.int32)).to(l.device)
        self.arc_parameters, self.ranks = None, np.zeros((arcs, K), dtype=np.int64)
        setup = None
        if model.parameters is not None:
            setup = _ArcSetup(observations, model, plain=True)
            u, Kc, units = setup.u, setup.Kc, arcs * setup.Kc
            C = engine.segment_products(V.reshape(rows * K, M), setup.Bt, seg, channels=K).reshape(rows, K, arcs, u)        # B~_a^T v
            C = (C.permute(2, 1, 0, 3) if setup.shared else C.sum(1, keepdim=True).permute(2, 1, 0, 3)).reshape(units, rows, u).contiguous()
            T, Y = torch.empty_like(C), torch.empty_like(C)
            engine.gemm_ex(C, setup.R_d, T)                                                              # R^T B~^T v, as rows
            engine.gemm_ex(T, setup.R_d, Y, transb=True)                                                 # the parameters of every row: R R^T B~^T v
            for a in range(arcs):
                a0, a1 = int(bounds[a]), int(bounds[a + 1])
                Ya = Y[a * Kc:(a + 1) * Kc]                                                              # [Kc, rows, u]
                engine.gemm_ex(Ya if setup.shared else Ya[0], setup.Bt[:, :, a0:a1].permute(1, 0, 2), V[:, :, a0:a1].permute(1, 0, 2), alpha=-1.0, beta=1.0)
                engine.gemm_ex(Ya[:, 0:1] if setup.shared else Ya[0, 0:1], setup.plain_Bt[:, :, a0:a1].permute(1, 0, 2), plain[:, None, a0:a1], alpha=-1.0,
                               beta=1.0)
            y = engine.to_host(Y[:, 0]).reshape(arcs, Kc, u)
            self.arc_parameters = y if setup.shared else y[:, 0]
            self.ranks = setup.ranks.reshape((arcs, Kc) if setup.shared else (arcs,))
        squares = engine.to_host(engine.segment_lag_products(V.reshape(rows * K, M), seg, 0)).reshape(rows, K, arcs)
        self.arcs = bounds[:-1].copy()
        self.arc_observation_counts = K * np.diff(bounds) - self.ranks.reshape(arcs, -1).sum(axis=1)
        self.arc_square_sums = squares[0].sum(axis=0)
        self.__traces = squares[1:].sum(axis=(0, 1)) / (rows - 1) if rows > 1 else None                   # (1 / S) sum_j |(I - Q_a Q_a^T) A~_a z_j|^2
        self.__rows, self.__seg = plain, seg                                                              # e^ [K, M] on the device, for covariance_function
        self.rows = V
        self.whitened = _like_input(V[0].t().contiguous(), self.__template)
        self.residuals = _like_input(plain.t().contiguous(), self.__template)
        self.__solution = self.__vectors = None
        self._bind(observations, model, block_points, setup, windows is not None)
        return self

    def _leverage_operands(self, normals, elimination):
        """every check of leverages(), on the host: returns (factor block, kept columns of the arcs or None)"""
        if self.__bound is None:
            raise ValueError('the leverages need the pass of an of_* call')
        observations, model, _, setup, temporal = self.__bound
        matrix = normals.matrix
        if temporal or matrix.shape != (1, 1):
            raise ValueError('leverages: a normal matrix of several blocks (TemporalParameters) is out of scope: a one-block matrix is '
                             'expected, got {0} x {1} blocks'.format(*matrix.shape))
        if normals.status != 'cholesky_factor' or matrix._holds_factor_inverses:
            raise ValueError('leverages: the matrix holds {0}: solve the system first (status cholesky_factor)'.format(
                'the inverses of the factor blocks' if normals.status == 'cholesky_factor' else normals.status))
        if matrix._extent() != (observations.P, observations.P):
            raise ValueError('leverages: the system has {0} x {1} parameters, the observations {2}'.format(*matrix._extent(), observations.P))
        columns = None
        if model.parameters is not None:
            elimination = normals.arc_elimination if elimination is None else elimination
            if elimination is None:
                raise ValueError('leverages: the fit is one under ArcParameters: pass elimination=ne.arc_elimination of its own system')
            columns = elimination._columns()
            if columns is None:
                raise ValueError('leverages: the hat matrix needs the eliminated columns: build with ArcParameters(keep=True)')
            if setup is not None and tuple(columns.shape) != (observations.P, setup.arcs * setup.Kc * setup.u):
                raise ValueError('leverages: the elimination holds columns {0}, this fit has {1} arcs of {2} x {3} parameters'.format(
                    tuple(columns.shape), setup.arcs, setup.Kc, setup.u))
        return matrix.device_block(0, 0), columns

    def __hat_diagonal(self, normals, elimination):
        """h [K, M] on the device; kept for the next call with the same system (redundancies, then standardised), which is held
        weakly; callers get copies, never this tensor"""
        factor, columns = self._leverage_operands(normals, elimination)
        key = (weakref.ref(normals), None if elimination is None else weakref.ref(elimination), factor.data_ptr())
        if self.__hat is not None and self.__hat[0][0]() is normals and self.__hat[0][2] == key[2] and \
                (elimination is None if self.__hat[0][1] is None else self.__hat[0][1]() is elimination):
            return self.__hat[1]
        torch = engine.require_gpu()
        observations, model, block_points, setup, _ = self.__bound
        P, K, M = observations.P, observations.K, observations.M
        Ui = engine.trtri(factor)
        h = torch.empty((K, M), dtype=torch.float64, device=factor.device)
        Q = q2 = None
        if setup is not None:
            # q_i = R_a^T b~_i for every observation: Q [u, K, M], by arc; |q_i|^2 is the part of the hat matrix the arc parameters take
            Q = torch.empty_like(setup.Bt)
            u, Kc = setup.u, setup.Kc
            for a in range(setup.arcs):
                a0, a1 = int(setup.bounds[a]), int(setup.bounds[a + 1])
                if a1 > a0:
                    Ra = setup.R_d[a * Kc:(a + 1) * Kc] if setup.shared else setup.R_d[a]
                    engine.gemm_ex(Ra, setup.Bt[:, :, a0:a1].permute(1, 0, 2), Q[:, :, a0:a1].permute(1, 0, 2), transa=True)
            flat = Q.reshape(u, K * M)
            q2 = engine.column_dots(flat, flat).reshape(K, M)
        for first, last, At, _, _, _ in _design_blocks(observations, model, block_points):
            Mb = last - first
            if setup is not None:
                # At~ -= D_a Q_a^T for the arcs that meet the block: the rows of (I - Q Q^T) A~
                At3 = At.reshape(P, K, Mb)
                u, Kc = setup.u, setup.Kc
                a_first = int(np.searchsorted(setup.bounds, first, side='right')) - 1
                for a in range(a_first, setup.arcs):
                    a0, a1 = max(int(setup.bounds[a]), first), min(int(setup.bounds[a + 1]), last)
                    if a0 >= last:
                        break
                    if a1 <= a0:
                        continue
                    D = columns[:, a * Kc * u:(a + 1) * Kc * u]
                    D = D.reshape(P, Kc, u).permute(1, 0, 2) if setup.shared else D
                    engine.gemm_ex(D, Q[:, :, a0:a1].permute(1, 0, 2), At3[:, :, a0 - first:a1 - first].permute(1, 0, 2), alpha=-1.0, beta=1.0)
            h[:, first:last] = engine.leverages(Ui, At).reshape(K, Mb)
        if q2 is not None:
            h += q2
        self.__hat = (key, h)
        return h

    def leverages(self, normals, elimination=None):
        """
        h [M, K], the diagonal of the hat matrix: h_i = a~_i^T N^-1 a~_i for every whitened, weighted row a~_i of the design matrix, a
        device tensor where the positions were one and a host array otherwise.  normals is a solved
        NormalEquations (status 'cholesky_factor') with a one-block matrix over the parameters of this fit: the group's own system
        or a combined one from accumulate_normals, regularisation included (the rows are taken as this fit whitened and weighted
        them: a group that entered the combination with a variance factor s^2 has the leverages h / s^2).  U^-1 comes from
        engine.trtri of its factor block, once per call, then one more pass over the design blocks of the fit with engine.leverages
        per block; under a noise model the rows are the whitened ones, with the halo of every block as in the pass.

        Under ArcParameters the hat matrix of the full model [A~ B~] is P_B + (I - P_B) A~ N^-1 A~^T (I - P_B) with P_B = Q Q^T,
        Q_a = B~_a R_a as the elimination forms them: h_i = |q_i|^2 + |U^-T (a~_i - D_a q_i)|^2 with the D_a that
        ArcParameters(keep=True) retains.  elimination defaults to normals.arc_elimination; a combined system has none, pass the
        one of this group's own system.

        The fit keeps the last h [K, M] on the device (K M doubles) for a following redundancies() or standardised() with the same
        system, which it refers to weakly; every call returns a tensor or array of its own.

        ValueError, before anything reaches the device: a matrix of several blocks (TemporalParameters is out of scope), a status
        other than 'cholesky_factor', a parameter count that does not match, an ArcParameters fit without kept columns.
        """
        return _like_input(self.__hat_diagonal(normals, elimination).t().clone(memory_format=engine._torch().contiguous_format), self.__template)

    def redundancies(self, normals, elimination=None):
        """r = 1 - h [M, K] of leverages(); their sum is the redundancy of the adjustment when the normals are the group's own"""
        return _like_input((1.0 - self.__hat_diagonal(normals, elimination)).t().contiguous(), self.__template)

    def standardised(self, normals, sigma=None, factors=None, elimination=None):
        """
        t = |e~| / (sqrt(f) sigma sqrt(r)) [M, K], the standardised residual of every observation: e~ is `whitened`, r the
        redundancies of the same arguments; sigma defaults to sqrt(sum e~^2 / (normals.observation_count - parameters)); factors
        [M] or [M, K] (default 1) are the Huber factors the weights of this fit already hold, so that t measures the residual
        against the standard deviation of the observation before its downweighting (the reference's loss_argument).  nan where
        r <= 0.  Device tensor or host array as `whitened`.
        """
        h = self.__hat_diagonal(normals, elimination)
        torch = engine.require_gpu()
        e = self.rows[0]
        if sigma is None:
            freedom = normals.observation_count - self.__bound[0].P
            if freedom <= 0:
                raise ValueError('standardised: {0} observations do not determine sigma beside {1} parameters'.format(
                    normals.observation_count, self.__bound[0].P))
            sigma = float(torch.sqrt((e * e).sum() / freedom).item())
        scale = float(sigma)
        r = 1.0 - h
        usable = r > 0
        t = e.abs() / (scale * torch.sqrt(torch.where(usable, r, torch.ones_like(r))))
        if factors is not None:
            f = engine.to_device(factors, e.device) if not _is_tensor(factors) else factors.to(e.device)
            f = f.reshape(f.shape[0], -1).to(torch.float64)
            t = t / torch.sqrt(f.t().expand_as(t) if f.shape[1] == t.shape[0] else f.t().expand(t.shape[0], -1))
        t = torch.where(usable, t, torch.full_like(t, float('nan')))
        return _like_input(t.t().contiguous(), self.__template)

    def arc_redundancies(self, variance_factor=1.0):
        """r_a = n_a - (1 / S) sum_j |(I - Q_a Q_a^T) A~_a z_j|^2 / variance_factor [arcs]: the estimator of NormalEquations.redundancy,
        restricted to the arc.  ValueError without vectors."""
        if self.__traces is None:
            raise ValueError('the redundancies of the arcs need the Monte-Carlo vectors: pass vectors=ne.monte_carlo_vectors')
        return self.arc_observation_counts - self.__traces / variance_factor

    def arc_variance_factors(self, variance_factor=1.0):
        """Omega_a / r_a [arcs], the arc-wise form of compute_variance_factors; nan where r_a <= 0"""
        redundancies = self.arc_redundancies(variance_factor)
        usable = redundancies > 0
        return np.where(usable, self.arc_square_sums / np.where(usable, redundancies, 1.0), np.nan)

    def covariance_function(self, maximum_lag, per_component=False, biased=True):
        """
        Empirical covariance function of the unwhitened residuals, c_k = sum_a sum_t e^[t] e^[t + k] / d_k over the pairs inside an arc
        (one call of shg_segment_lag_products), k = 0 .. maximum_lag <= 128.  biased=True: d_k = d_0 = sum_a len_a, positive
        semi-definite by construction; biased=False: d_k = sum_a max(len_a - k, 0).  The components are pooled into one function
        (K d_k in the divisor), or per_component=True gives one function each.  Returns what
        AutoregressiveModelSequence.from_covariance_function takes, a list of [1, 1] arrays, or a list of K such lists.  ValueError
        for a maximum_lag outside 0 .. 128 and, with biased=False, for a lag no arc is long enough for.  covariance_lags gives the
        same numbers as arrays, up to lag 4095.
        """
        _check_maximum_lag(maximum_lag, MAX_WHITENING_ORDER)
        c = self.__covariance(int(maximum_lag), per_component, biased)
        if per_component:
            return [[np.array([[value]]) for value in row] for row in c]
        return [np.array([[value]]) for value in c]

    def __pairs(self, q, biased):
        """d_k [q + 1] of covariance_function and cross_covariance_function, on the host"""
        lengths = np.diff(np.append(self.arcs, int(self.__rows.shape[1])))
        pairs = np.array([np.maximum(lengths - k, 0).sum() for k in range(q + 1)], dtype=np.float64)
        if biased:
            pairs[:] = pairs[0]
        elif not np.all(pairs > 0):
            raise ValueError('no arc is longer than {0} points: no pair at lag {1}'.format(int(lengths.max()), int(np.argmin(pairs > 0))))
        return pairs

    def __covariance(self, q, per_component, biased):
        """c [q + 1] or [K, q + 1] of covariance_function and covariance_lags; up to lag 128 shg_segment_lag_products, beyond it
        shg_segment_lag_products_long"""
        pairs = self.__pairs(q, biased)
        products = engine.segment_lag_products if q <= MAX_WHITENING_ORDER else engine.segment_lag_products_long
        sums = engine.to_host(products(self.__rows, self.__seg, q)).sum(axis=1)                           # [K, q + 1]
        if per_component:
            return sums / pairs
        return sums.sum(axis=0) / (sums.shape[0] * pairs)

    def covariance_lags(self, maximum_lag, per_component=False, biased=True):
        """
        The numbers of covariance_function as plain arrays, ndarray [q + 1] or, with per_component, [K, q + 1], for
        0 <= maximum_lag <= MAX_COVARIANCE_ORDER = 4095: the same divisors, pooling and meaning of `biased`.  Up to lag 128 it is
        bitwise covariance_function (shg_segment_lag_products); beyond, the sums run on the fp64 MFMA
        (shg_segment_lag_products_long), which needs finite residuals.  ValueError, before anything reaches
        the device, for a maximum_lag that is no integer in 0 .. 4095 and, with biased=False, for a lag no arc is long enough for.
        """
        _check_maximum_lag(maximum_lag, MAX_COVARIANCE_ORDER)
        return self.__covariance(int(maximum_lag), per_component, biased)

    def covariance_model(self, maximum_lag, per_component=False, window=None):
        """
        The noise model of the residuals: a CovarianceFunction of the biased covariance_lags(maximum_lag), or a list of K of them
        with per_component, for ColouredNoise, ArcParameters(noise_model=), TemporalParameters(model=) and RadialBasisParameters.
        The biased estimate is a sum of positive semi-definite sequences, so the Levinson-Durbin recursion accepts it unless the
        residuals are degenerate; a CovarianceFunction that is not positive definite raises its own ValueError.  window tapers the
        lags on the host first, c_k w_k with lag_window(window, maximum_lag): None, 'bartlett', 'parzen' (both positive
        semi-definite, so the product stays so) or an array [q + 1] with w_0 = 1.  ValueError for any other window and for the
        maximum_lag, before anything reaches the device.
        """
        _check_maximum_lag(maximum_lag, MAX_COVARIANCE_ORDER)
        taper = lag_window(window, int(maximum_lag))
        c = self.__covariance(int(maximum_lag), per_component, True) * taper
        return [CovarianceFunction(row) for row in c] if per_component else CovarianceFunction(c)

    def __cross_covariance(self, maximum_lag, biased):
        """Sigma [q + 1, K, K] of cross_covariance_function; its checks on the host first"""
        _check_maximum_lag(maximum_lag, MAX_WHITENING_ORDER)
        q, K = int(maximum_lag), int(self.__rows.shape[0])
        if K > MAX_VECTOR_DIMENSION:
            raise ValueError('cross-covariances of {0} components: at most {1}'.format(K, MAX_VECTOR_DIMENSION))
        pairs = self.__pairs(q, biased)
        sums = engine.to_host(engine.segment_cross_lag_products(self.__rows, self.__seg, q)).sum(axis=0)      # [q + 1, K, K]
        return sums / pairs[:, None, None]

    def cross_covariance_function(self, maximum_lag, biased=True):
        """
        Empirical cross-covariance function of the K components of the unwhitened residuals,
        Sigma_k[c, c'] = sum_a sum_t e^[t, c] e^[t + k, c'] / d_k over the pairs inside an arc (one call of
        shg_segment_cross_lag_products), k = 0 .. maximum_lag <= 128, with the divisors of covariance_function: biased=True
        d_k = d_0 = sum_a len_a, positive semi-definite as a block sequence by construction; biased=False d_k = sum_a max(len_a - k, 0).
        Returns a list of q + 1 [K, K] arrays, Sigma_k = E[x_t x_(t+k)^T]: what AutoregressiveModelSequence.from_covariance_function
        takes.  The diagonal entries are covariance_function(per_component=True).  ValueError, before anything reaches the device,
        for a maximum_lag outside 0 .. 128, more than 6 components and, with biased=False, a lag no arc is long enough for.
        """
        return list(self.__cross_covariance(maximum_lag, biased))

    def vector_noise(self, maximum_lag, window=None):
        """
        The vector noise model of the residuals, the counterpart of covariance_model for components that are correlated: the
        VectorNoise of AutoregressiveModelSequence.from_covariance_function (block Yule-Walker systems on the device) of the biased
        cross_covariance_function(maximum_lag), every lag tapered by lag_window(window, maximum_lag) first; for ColouredNoise,
        ArcParameters(noise_model=), TemporalParameters(model=), RadialBasisParameters and decorrelate.  ValueError for the window, the
        maximum_lag and fewer than 2 components before anything reaches the device; VectorNoise raises its own for an estimate that
        is not positive definite.
        """
        _check_maximum_lag(maximum_lag, MAX_WHITENING_ORDER)
        K = int(self.__rows.shape[0])
        if not MIN_VECTOR_DIMENSION <= K <= MAX_VECTOR_DIMENSION:
            raise ValueError('vector noise of {0} component{1}: expected {2} .. {3} (covariance_model gives the scalar model)'.format(
                K, '' if K == 1 else 's', MIN_VECTOR_DIMENSION, MAX_VECTOR_DIMENSION))
        taper = lag_window(window, int(maximum_lag))
        lags = self.__cross_covariance(maximum_lag, True) * taper[:, None, None]
        return VectorNoise(AutoregressiveModelSequence.from_covariance_function([np.ascontiguousarray(lag) for lag in lags]))


def _check_maximum_lag(maximum_lag, most):
    if int(maximum_lag) != maximum_lag or not 0 <= maximum_lag <= most:
        raise ValueError('maximum_lag must be an integer in 0 .. {0}, got {1!r}'.format(most, maximum_lag))


def lag_window(window, maximum_lag):
    """
    w [q + 1], the taper of the lags 0 .. q = maximum_lag of an estimated covariance function (host, NumPy only), w_0 = 1:
    None: all ones.  'bartlett': w_k = 1 - k / (q + 1).  'parzen': with m = q + 1, w_k = 1 - 6 (k/m)^2 + 6 (k/m)^3 for k <= m / 2 and
    2 (1 - k/m)^3 above.  Both are positive semi-definite sequences, so they keep an estimate positive semi-definite.  An array
    [q + 1] with w_0 = 1 is taken as given.  ValueError for anything else.
    """
    q = int(maximum_lag)
    if window is None:
        return np.ones(q + 1)
    if isinstance(window, str):
        x = np.arange(q + 1) / (q + 1.0)
        if window == 'bartlett':
            return 1.0 - x
        if window == 'parzen':
            return np.where(x <= 0.5, 1.0 - 6.0 * x * x + 6.0 * x * x * x, 2.0 * (1.0 - x) ** 3)
        raise ValueError("window must be None, 'bartlett', 'parzen' or an array of {0} weights, got {1!r}".format(q + 1, window))
    try:
        w = np.array(window, dtype=np.float64)
    except (TypeError, ValueError):
        w = None
    if w is None or w.shape != (q + 1,) or not np.all(np.isfinite(w)) or w[0] != 1.0:
        raise ValueError("window must be None, 'bartlett', 'parzen' or an array of {0} finite weights with w_0 = 1".format(q + 1))
    return w


def accumulate_normals(normal_equations, variance_factors):
    """Weighted sum of normal equation systems, N = sum_k N_k / s_k^2 (same for the right-hand side and l^T P l); the observation
    counts add up unweighted (grates/lstsq.py:1091-1119)."""
    # as the reference: one factor per system is read (further factors are ignored, a missing one is an IndexError), the matrix is scaled
    # by the reciprocal, right-hand side and square sum are DIVIDED by the factor (bit-equal to grates/lstsq.py:1106-1116)
    factors = [variance_factors[k] for k in range(len(normal_equations))]
    matrix = normal_equations[0].matrix.copy()
    matrix._scale(1 / factors[0])
    for part, factor in zip(normal_equations[1:], factors[1:]):
        matrix._axpy(1 / factor, part.matrix)
    sides = [engine.to_host(part.right_hand_side) if _is_tensor(part.right_hand_side) else part.right_hand_side for part in normal_equations]
    right_hand_side = sides[0].copy() / factors[0]
    square_sum = normal_equations[0].observation_square_sum / factors[0]
    for part, side, factor in zip(normal_equations[1:], sides[1:], factors[1:]):
        right_hand_side += side / factor
        square_sum += part.observation_square_sum / factor
    count = sum(part.observation_count for part in normal_equations)
    return NormalEquations(matrix, right_hand_side, square_sum, count)


def compute_variance_factors(normal_equations, combined_normals, solution, variance_factors):
    """Variance component estimates of the individual systems (grates/lstsq.py:1122-1149)."""
    return np.array([part.residual_square_sum(solution) / part.redundancy(combined_normals, factor)
                     for part, factor in zip(normal_equations, variance_factors)])


def huber_factors(standardised, redundancies, factors=None, threshold=2.5, downweight_power=1.5, redundancy_threshold=1e-4):
    """
    One step of the Huber reweighting: (new_factors, outliers) from the standardised residuals t and the redundancies r of every
    observation (PostFit.standardised, PostFit.redundancies; host arrays or device tensors of one shape, [M, K] or [k]).  An
    observation is flagged where t is finite, t > threshold and r > redundancy_threshold, and a flagged observation gets the weight
    factor f = (threshold / t)^(2 downweight_power): the reference's std_dev = (t / threshold)^downweight_power, applied as
    1 / std_dev^2 (grates/lstsq.py:1362-1363).  An observation that is not flagged keeps its earlier factor (`factors`, default 1), as
    in the reference.  The factors multiply the base weights of the observations.

    factors has the shape of t, [M, K], where the kind of observation takes weights per component; for a kind that takes weights
    per point only (line of sight, potentials, potential differences), or weights given per point, pass factors [M]: the new factor
    of a point is then the smallest over its components, flagged components at (threshold / t)^(2 downweight_power) and the others
    at the earlier factor of the point.  outliers always has the shape of t.
    """
    tensor = _is_tensor(standardised)
    xp = engine._torch() if tensor else np
    t = standardised if tensor else np.asarray(standardised, dtype=np.float64)
    r = redundancies if tensor else np.asarray(redundancies, dtype=np.float64)
    if tuple(t.shape) != tuple(r.shape):
        raise ValueError('huber_factors: standardised {0} and redundancies {1} must have one shape'.format(tuple(t.shape), tuple(r.shape)))
    if not (threshold > 0 and downweight_power > 0):
        raise ValueError('huber_factors: threshold and downweight_power must be positive')
    if factors is None:
        f = xp.ones_like(t)
    elif tensor:
        f = (factors if _is_tensor(factors) else engine.to_device(np.asarray(factors, dtype=np.float64))).to(device=t.device, dtype=t.dtype)
    else:
        f = np.asarray(engine.to_host(factors) if _is_tensor(factors) else factors, dtype=np.float64)
    per_point = f.ndim == t.ndim - 1
    if tuple(f.shape) != (tuple(t.shape[:-1]) if per_point else tuple(t.shape)):
        raise ValueError('huber_factors: factors {0} fit neither {1} nor {2}'.format(tuple(f.shape), tuple(t.shape), tuple(t.shape[:-1])))
    outliers = xp.isfinite(t) & (t > threshold) & (r > redundancy_threshold)
    safe = xp.where(outliers, t, xp.ones_like(t))                      # (no nan, inf or zero reaches the power)
    earlier = f[..., None] if per_point else f
    new = xp.where(outliers, (threshold / safe) ** (2.0 * downweight_power), earlier + xp.zeros_like(t))
    if per_point:
        new = new.min(dim=-1).values if tensor else new.min(axis=-1)
    return new, outliers


# The factors "no longer change" within this, relative.  With stable flags the loop contracts by about 0.02 per iteration (the factors
# depend on each other through sigma0 alone), so bitwise repetition takes longer than the reference's ten iterations; sigma0 itself is
# known to 1 / sqrt(2 (k - p)), a few percent, and a factor that moves by 1e-6 of itself changes nothing a weight means.
HUBER_TOLERANCE = 1e-6


def _huber_settled(factors, flags, new_factors, new_flags):
    if flags is None or factors is None:
        return False
    xp = engine._torch() if _is_tensor(new_factors) else np
    return bool((flags == new_flags).all()) and bool((xp.abs(new_factors - factors) <= HUBER_TOLERANCE * xp.abs(factors)).all())


def huber_iterate(system, post_fit, weights, threshold=2.5, downweight_power=1.5, redundancy_threshold=1e-4, max_iter=10):
    """
    The solve, reweight loop per observation: system(w) returns the NormalEquations under the weights w,
    post_fit(x, w, ne) the PostFit of the solution x [P, 1] under the same weights and model, e.g.

        system = lambda w: model.from_accelerations(xyz, g, 2, 96, weights=w)
        post_fit = lambda x, w, ne: PostFit.of_accelerations(x, xyz, g, 2, 96, weights=w, model=model)

    weights [M] or [M, K] (host array; None: 1) are the base weights.  Every iteration solves the system under weights * factors,
    takes t = post_fit.standardised(ne, factors=factors) and r = post_fit.redundancies(ne) and the new factors and flags from
    huber_factors.  It stops when the flags are the same and the factors agree within 1e-6 of themselves (HUBER_TOLERANCE) with those of the
    iteration before, or after max_iter solutions.  Returns (x, ne, factors, outliers) of the last solution: x and ne belong to
    the factors of the iteration before, which are the returned ones where the loop stopped by itself; factors has the shape of
    weights (without weights: [M, K], or [M] for K = 1), outliers [M, K]; both are host arrays.

    Under a noise model the residual and the leverage are those of the decorrelated rows, and the factor goes to the weight of the
    sample with the same index: a spike in one sample spreads over the q samples behind it in the decorrelated series, so the
    neighbours of an outlier may be flagged with it.  That is the usual approximation.
    """
    base = None if weights is None else np.asarray(engine.to_host(weights) if _is_tensor(weights) else weights, dtype=np.float64)
    if int(max_iter) < 1:
        raise ValueError('huber_iterate: max_iter must be at least 1')
    factors = flags = x = ne = None
    for _ in range(int(max_iter)):
        w = base if factors is None else (factors if base is None else base * factors)
        ne = system(w)
        x = ne.solve()
        fit = post_fit(x, w, ne)
        t = fit.standardised(ne, factors=factors)
        r = fit.redundancies(ne)
        t, r = (engine.to_host(v) if _is_tensor(v) else v for v in (t, r))
        if factors is None:
            shape = base.shape if base is not None else (t.shape if t.shape[1] > 1 else t.shape[:1])
            earlier = np.ones(shape)
        else:
            earlier = factors
        new_factors, new_flags = huber_factors(t, r, earlier, threshold, downweight_power, redundancy_threshold)
        settled = _huber_settled(factors if factors is not None else earlier, flags if flags is not None else np.zeros_like(new_flags),
                                 new_factors, new_flags)
        factors, flags = new_factors, new_flags
        if settled:
            break
    return x, ne, factors, flags


def robust_least_squares(l, A, threshold=2.5, downweight_power=1.5, redundancy_threshold=1e-4, max_iter=10):
    """
    Iterative robust least squares adjustment with the Huber estimator (grates/lstsq.py:1320-1365: the same arguments and the same
    return triple) for explicit observations l [k] and a design matrix A [k, p], host arrays or device tensors.

    Returns x_hat [p], C [p, p] = sigma0^2 N^-1 and outlier_flag [k] (bool) of the last iteration, host arrays or device tensors as A.
    As in the reference x_hat and C are those of the weights the last iteration started with, and an observation that is not
    flagged keeps the factor it has.

    Every iteration runs on the device: the rows are scaled by sqrt(f), N = A~^T A~ and n = A~^T l~ on engine.gemm, the factor by
    engine.potrf, U^-1 by engine.trtri, x_hat = U^-1 U^-T n, the leverages a~_i^T N^-1 a~_i by engine.leverages on A~^T, then
    huber_factors.  Unlike the reference, which always runs max_iter iterations, the loop ends as soon as the flags are those of the
    iteration before and every factor agrees with its predecessor within HUBER_TOLERANCE = 1e-6 of itself -- not bitwise: what comes
    back may be the solution of an earlier iteration than the reference's last, and differs from it by what a relative change of 1e-6 in
    the weights of the flagged observations moves (below 1e-9 of x_hat in the tests' problems, by the argument at HUBER_TOLERANCE,
    not by a derived bound).  max_iter iterations are never exceeded.

    This is the textbook estimator: weights 1 / std_dev^2, redundancy r_i = 1 - a~_i^T N^-1 a~_i, standardised residual
    |e~_i| std_dev_i / (sigma0 sqrt(r_i)).  The body of the reference does something else: it inverts A_bar^T A (one factor of
    1 / std_dev, not two) and takes 1 - sum(A_bar^2, axis=1) as the redundancy, which is the diagonal of the hat matrix only for
    orthonormal columns and unit weights.  The two agree in that setting at max_iter=1 (tests/golden/g32_robust.npz) and nowhere
    else; the reference's formulas are not mirrored.
    """
    torch = engine.require_gpu()
    host = not _is_tensor(A)
    At = _dev(A).t().contiguous()                                                                  # [p, k]
    p, k = int(At.shape[0]), int(At.shape[1])
    lt = _dev(l).reshape(-1)
    if int(lt.shape[0]) != k:
        raise ValueError('robust_least_squares: l has {0} entries, A {1} rows'.format(int(lt.shape[0]), k))
    if k <= p:
        raise ValueError('robust_least_squares: {0} observations do not determine sigma0 beside {1} parameters'.format(k, p))
    if int(max_iter) < 1:
        raise ValueError('robust_least_squares: max_iter must be at least 1')
    factors, flags = torch.ones(k, dtype=torch.float64, device=At.device), torch.zeros(k, dtype=torch.bool, device=At.device)
    for _ in range(int(max_iter)):
        root = torch.sqrt(factors)
        Aw, lw = At * root, (lt * root).reshape(k, 1)
        N = engine.gemm(Aw, Aw, transb=True)
        n = engine.gemm(Aw, lw)
        Ui = engine.trtri(engine.potrf(N))
        x = engine.gemm(Ui, engine.gemm(Ui, n, transa=True))
        e = (lw - engine.gemm(Aw, x, transa=True)).reshape(k)
        r = 1.0 - engine.leverages(Ui, Aw)
        variance = (e * e).sum() / (k - p)
        usable = r > 0
        t = e.abs() / (root * torch.sqrt(variance) * torch.sqrt(torch.where(usable, r, torch.ones_like(r))))
        t = torch.where(usable, t, torch.full_like(t, float('nan')))
        C = engine.gemm(Ui, Ui, transb=True) * variance
        new_factors, new_flags = huber_factors(t, r, factors, threshold, downweight_power, redundancy_threshold)
        settled = _huber_settled(factors, flags, new_factors, new_flags)
        factors, flags = new_factors, new_flags
        if settled:
            break
    x = x.reshape(p)
    return (engine.to_host(x), engine.to_host(C), flags.cpu().numpy()) if host else (x, C, flags)


class UnscentedTransformSymmetric:
    """
    Unscented transform on the symmetric sigma point set of Julier and Uhlmann (Proc. IEEE 92, 2004), grates/lstsq.py:1152-1250: the
    same constructor, set_size, weights(), sigma_points, average and sigma_point_covariance.  dim: dimension of the random variable
    (the number of eigenpairs used), w0 < 1: the weight of the central point.  Arrays may be NumPy arrays (NumPy results) or device
    tensors (device results); the products run on engine.gemm.

    One deviation: the reference adds +sqrt(dim / (1 - w0)) sqrt(lambda_i) v_i for BOTH halves of the set (its scale vector has no
    negative entries), so its points are not symmetric and their weighted mean is not x0.  Here the second half has the minus sign
    of the paper: average(sigma_points(x0, ...)) is x0, and sigma_point_covariance of the deviations from it is V diag(lambda) V^T.
    """

    def __init__(self, dim, w0):
        self.w0 = w0
        self.dim = dim
        self.__w = np.full(self.set_size, 0.5 * (1 - self.w0) / self.dim)
        self.__w[0] = self.w0
        self.__s = np.full(self.set_size, np.sqrt(self.dim / (1 - self.w0)))
        self.__s[0] = 0
        self.__s[self.dim + 1:] *= -1.0

    @property
    def set_size(self):
        """the number of sigma points, 2 dim + 1"""
        return 2 * self.dim + 1

    def weights(self):
        """the weights of the mean and of the covariance (the same NumPy vector [2 dim + 1] twice, as in the reference)"""
        return self.__w, self.__w

    def sigma_points(self, x0, eigen_values, eigen_vectors):
        """S [n, 2 dim + 1] = x0, x0 + s sqrt(lambda_i) v_i, x0 - s sqrt(lambda_i) v_i (i < dim, s = sqrt(dim / (1 - w0))) for the mean
        x0 [n], eigenvalues [p] and eigenvectors [n, p] with p >= dim, as teigh returns them: one broadcast on the device"""
        n, p = tuple(eigen_vectors.shape)
        if int(x0.shape[0]) != n or int(eigen_values.shape[0]) != p or p < self.dim:
            raise ValueError('sigma_points: x0 {0}, eigenvalues {1} and eigenvectors {2} do not fit dimension {3}'.format(
                tuple(x0.shape), tuple(eigen_values.shape), (n, p), self.dim))
        torch = engine.require_gpu()
        pick = torch.arange(self.set_size, device=engine.device())
        pick = (torch.where(pick > self.dim, pick - self.dim, pick) - 1).clamp_min(0)  # the eigenpair of every point (the centre: any)
        s = engine.to_device(self.__s)
        scale = torch.where(s == 0.0, s, s * torch.sqrt(_dev(eigen_values))[pick])     # the centre has s = 0
        return _like_input(_dev(x0).reshape(n, 1) + _dev(eigen_vectors)[:, pick] * scale, x0)

    def average(self, sigma_points):
        """x [n] = sum_j w_j S[:, j]"""
        w, _ = self.weights()
        return _like_input(engine.gemm(_dev(sigma_points), engine.to_device(w).reshape(-1, 1)).reshape(-1), sigma_points)

    def sigma_point_covariance(self, sigma_points):
        """C [n, n] = (S * w) S^T (not centred, as in the reference: pass deviations from the mean for a covariance about it)"""
        _, w = self.weights()
        S = _dev(sigma_points)
        return _like_input(engine.gemm(S * engine.to_device(w), S, transb=True), sigma_points)


TEIGH_BLOCK = engine.JACOBI_MAX        # width of the iterated subspace of teigh (the Rayleigh-Ritz problem must fit engine.syev)
TEIGH_OVERSAMPLING = 16                # columns of that subspace beyond the wanted pairs, at least
_DEFAULT_SEED = 20040301


def _device_generator(generator, device):
    """a torch generator on `device`: `generator` itself when it is one, else seeded from it (an int, a numpy Generator or
    RandomState, a torch generator of another device) or, for None, from a fixed default so that calls repeat"""
    torch = engine._torch()
    if isinstance(generator, torch.Generator) and generator.device == device:
        return generator
    if generator is None:
        seed = _DEFAULT_SEED
    elif isinstance(generator, torch.Generator):
        seed = generator.initial_seed()
    elif isinstance(generator, np.random.Generator):
        seed = int(generator.integers(2 ** 62))
    elif isinstance(generator, np.random.RandomState):
        seed = int(generator.randint(2 ** 31 - 1))
    else:
        seed = int(generator)
    return torch.Generator(device=device).manual_seed(seed)


def _check_count(name, what, count, most):
    if int(count) != count or not 1 <= int(count) <= most:
        raise ValueError('{0}: {1} {2} is outside 1 .. {3}'.format(name, what, count, most))
    return int(count)


def teigh(M, eigenvalue_count, tolerance=1e-12, max_iter=100, generator=None):
    """
    Truncated eigenvalue decomposition of a symmetric matrix (grates/lstsq.py:1253-1274): the eigenvalue_count largest eigenvalues
    w [k], descending, and their eigenvectors v [n, k], NumPy arrays or device tensors as M.  Like the reference (lower=False) the
    strict lower triangle of M is never read.

    n <= 128: all eigenpairs by engine.syev (Jacobi rotations in LDS), of which the top k are returned; tolerance, max_iter and
    generator play no part.  n > 128: block subspace iteration with Rayleigh-Ritz extraction on a block of 128 columns, k <= 112
    (ValueError above: at least 16 columns oversample).  Q = orthonormalise(randn(n, 128)); then Y = M Q on the fp64 MFMA (M
    mirrored once into a work copy), H = Q^T Y, its eigenpairs by engine.syev, the k largest Ritz pairs (theta_i, v_i = Q s_i); it
    ends when max_i |M v_i - theta_i v_i|_2 <= tolerance |M|_F and continues with Q = orthonormalise(Y) otherwise.
    numpy.linalg.LinAlgError after max_iter iterations without convergence, and from orthonormalise when M Q is numerically rank
    deficient (rank of M below 128: no eigenvalue decay left to iterate on).  The iteration finds the eigenvalues of largest
    magnitude; they are the largest ones for the positive semi-definite matrices (covariances, normals) this is meant for.
    generator: an int seed, a numpy or torch generator, or None for a fixed seed; the same seed gives the same result.
    """
    shape = tuple(int(s) for s in M.shape)
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError('teigh: a square matrix is expected, got shape {0}'.format(shape))
    n = shape[0]
    k = _check_count('teigh', 'eigenvalue_count', eigenvalue_count, n)
    if n > engine.JACOBI_MAX and k > TEIGH_BLOCK - TEIGH_OVERSAMPLING:
        raise ValueError('teigh: eigenvalue_count {0} above {1} for a matrix wider than {2}'.format(k, TEIGH_BLOCK - TEIGH_OVERSAMPLING,
                                                                                                 engine.JACOBI_MAX))
    if int(max_iter) < 1:
        raise ValueError('teigh: max_iter must be at least 1')
    torch = engine.require_gpu()
    A = _dev(M)
    if n <= engine.JACOBI_MAX:
        w, v, _ = engine.syev(A)
        return _like_input(w[n - k:].flip(0), M), _like_input(v[:, n - k:].flip(1), M)
    _mirror_upper(A)
    norm = float(torch.linalg.norm(A).item())
    b = TEIGH_BLOCK
    Q = engine.orthonormalise(torch.randn((n, b), generator=_device_generator(generator, A.device), dtype=torch.float64, device=A.device))
    for _ in range(int(max_iter)):
        Y = engine.gemm(A, Q)
        H = engine.gemm(Q, Y, transa=True)
        theta, S, _ = engine.syev(0.5 * (H + H.t()))
        theta, S = theta[b - k:].flip(0), S[:, b - k:].flip(1)
        v = engine.gemm(Q, S)
        residual = float((engine.gemm(Y, S) - v * theta).norm(dim=0).max().item())
        if residual <= tolerance * norm:
            return _like_input(theta, M), _like_input(v, M)
        Q = engine.orthonormalise(Y)
    raise np.linalg.LinAlgError('teigh: residual {0:.3e} above {1:.3e} = tolerance |M|_F after {2} iterations'.format(
        residual, tolerance * norm, int(max_iter)))


def trsvd(A, singular_value_count, iteration_count=5, generator=None):
    """
    Randomized truncated singular value decomposition after Halko, Martinsson and Tropp (SIAM Review 53, 2011), the loop of
    grates/lstsq.py:1277-1314: Q = orth(A Omega) with a Gaussian Omega [n, k], then iteration_count rounds of Q = orth(A orth(A^T Q)),
    and the decomposition of B = Q^T A [k, n].  Returns U [m, k], s [k] descending and Vt [k, n], NumPy arrays or device tensors as A,
    with A ~ U diag(s) Vt.  k = singular_value_count <= min(m, n, 128), ValueError otherwise.

    Every product runs on the fp64 MFMA, every orth is engine.orthonormalise (shifted CholeskyQR3).  The small decomposition does not
    go through B B^T, which would square the condition number: B^T = Q2 R2 (orthonormalise, R2 = Q2^T B^T [k, k]), R2^T = Us S Vs^T by
    engine.jacobi_svd, U = Q Us, Vt = (Q2 Vs)^T.  The reference's numpy.linalg.svd(B) returns a full [n, n] Vt whose rows from k on
    are an arbitrary basis of the null space of B; those rows are not produced here.  numpy.linalg.LinAlgError (from
    orthonormalise) when the rank of A is numerically below k.
    generator: an int seed, a numpy or torch generator, or None for a fixed seed; the same seed gives the same result.
    """
    shape = tuple(int(s) for s in A.shape)
    if len(shape) != 2:
        raise ValueError('trsvd: a matrix is expected, got shape {0}'.format(shape))
    m, n = shape
    k = _check_count('trsvd', 'singular_value_count', singular_value_count, min(m, n, engine.JACOBI_MAX))
    if int(iteration_count) < 0:
        raise ValueError('trsvd: iteration_count must not be negative')
    torch = engine.require_gpu()
    Ad = _dev(A)
    omega = torch.randn((n, k), generator=_device_generator(generator, Ad.device), dtype=torch.float64, device=Ad.device)
    Q = engine.orthonormalise(engine.gemm(Ad, omega))
    for _ in range(int(iteration_count)):
        Q = engine.orthonormalise(engine.gemm(Ad, Q, transa=True))
        Q = engine.orthonormalise(engine.gemm(Ad, Q))
    Bt = engine.gemm(Ad, Q, transa=True)
    Q2 = engine.orthonormalise(Bt)
    R2 = engine.gemm(Q2, Bt, transa=True)
    Us, s, Vst, _ = engine.jacobi_svd(R2.t().contiguous())
    return _like_input(engine.gemm(Q, Us), A), _like_input(s, A), _like_input(engine.gemm(Vst, Q2, transb=True), A)
