"""Iteration observer (API of nsol/observer.py:21-161).

Two modes:

keep_iterates=True (the default, the reference's behaviour): the solvers hand
  the observer a host copy of every iterate (`add_x`); the measure callables
  are evaluated over that history by compute_measures().  Every iteration then
  costs a device-to-host copy of the iterate, and the fused solvers step one
  launch per iteration.

keep_iterates=False (device mode): the iterates stay on the device.  The
  solvers observe the start vector, iterations every, 2 every, ... and always
  the last one (get_observed_iterations()); at the start of run() each measure
  callable is called once with the symbolic probe (symbolic.Sym) and falls
  into one of four classes (get_measure_classes()):
    "board"      SSD, SAD, MAE, MSE, RMSE, PSNR, NCC, TK0, TK1, TV, Huber:
                 one pass of nsol_observe_* per distinct (reference, gradient,
                 gamma) writes their float64 sums into a device board;
    "ssim"       SSIM: nsol_ssim_* writes into a board slot;
    "histogram"  entropies, MI, NMI, Dice: the device functions of
                 similarity_measures.py on the float64 iterate (small
                 read-backs and a wait per observation, no copy of the iterate);
    "host"       anything else: called with a host copy at each observation.
  References are uploaded once per run.  The board is read once, after the
  solver's final synchronisation, and the values are ready when run() returns;
  compute_measures() only finalises; it also re-raises the first error of a
  histogram or host measure, which does not abort the solver's run (that
  measure's remaining points stay NaN).  get_x_list() stays empty.
"""
import numpy as np

from ._accessors import add_accessors
from .symbolic import MeasureDesc, Sym

BOARD_KINDS = ("SSD", "SAD", "MAE", "MSE", "RMSE", "PSNR", "NCC", "TK0", "TK1",
               "TV", "Huber")
PAIR_KINDS = ("SSD", "SAD", "MAE", "MSE", "RMSE", "PSNR", "NCC")
HIST_KINDS = ("entropy", "joint_entropy", "MI", "NMI", "Dice")


def observation_points(iterations, every):
    """Iterations observed by a run of `iterations` iterations: 0, every,
    2 every, ... and always the last."""
    iterations, every = int(iterations), int(every)
    pts = list(range(0, iterations + 1, every))
    if pts[-1] != iterations:
        pts.append(iterations)
    return pts


def classify(desc):
    """Class of a measure from what it answered the probe with."""
    if not isinstance(desc, MeasureDesc):
        return "host"
    if desc.kind in BOARD_KINDS:
        return "board"
    if desc.kind == "SSIM":
        return "ssim"
    if desc.kind in HIST_KINDS:
        return "histogram"
    return "host"


def probe_measure(fn, n):
    """fn applied to a flat length-n probe: its MeasureDesc or None."""
    try:
        out = fn(Sym((n,)))
    except Exception:
        return None
    return out if isinstance(out, MeasureDesc) else None


def reference_stats(y_sum, y_max, y_css, n):
    """Set-up constants of a reference y of n elements from its sum, maximum
    and centred sum of squares sum (y - ybar)^2."""
    ybar = y_sum / n
    return dict(n=float(n), mean=ybar, max=y_max, css=y_css,
                cs=y_sum - n * ybar)


def finalise(kind, s, ref=None):
    """Value of board measure `kind` from the 9 sums s of nsol_observe_* (see
    include/nsol_hip.h) and the reference's set-up constants `ref`
    (reference_stats; pair measures only)."""
    if kind == "TK0":
        return 0.5 * s[8]
    if kind == "TK1":
        return 0.5 * s[7]
    if kind == "TV":
        return float(s[5])
    if kind == "Huber":
        return float(s[6])
    n = ref["n"]
    if kind == "SSD":
        return float(s[0])
    if kind == "SAD":
        return float(s[1])
    if kind == "MAE":
        return float(s[1]) / n
    if kind == "MSE":
        return float(s[0]) / n
    if kind == "RMSE":
        return float(np.sqrt(float(s[0]) / n))
    if kind == "PSNR":
        mse = s[0] / n
        with np.errstate(divide="ignore"):
            return float(10 * np.log10(ref["max"] ** 2 / mse))
    if kind == "NCC":
        # sums about the reference's mean ybar, shifted to x's own mean:
        # sum (x - xbar)(y - ybar) = S3 - d sum (y - ybar),
        # sum (x - xbar)^2 = S4 - 2 d sum (x - ybar) + n d^2,   d = xbar - ybar
        ybar = ref["mean"]
        d = s[2] / n - ybar
        sxy = s[3] - d * ref["cs"]
        sxx = s[4] - 2.0 * d * (s[2] - n * ybar) + n * d * d
        sx = np.sqrt(sxx / (n - 1.0))
        sy = np.sqrt(ref["css"] / (n - 1.0))
        return float(sxy / (n * sx * sy))
    raise ValueError("not a board measure: %s" % kind)


class Observer(object):

    def __init__(self, name="Observer", keep_iterates=True, every=1):
        self._name = name
        self._computational_time = None
        self._x_list = []
        self._functions = {}        # measure name -> callable(x) -> float
        self._values = {}           # measure name -> np.ndarray over history
        self.set_keep_iterates(keep_iterates)
        self.set_every(every)
        self._session = None        # device mode: the last run's _DeviceRun

    def set_keep_iterates(self, keep):
        self._keep_iterates = bool(keep)

    def get_keep_iterates(self):
        return self._keep_iterates

    def set_every(self, every):
        every = int(every)
        if every < 1:
            raise ValueError("every must be a positive integer")
        self._every = every

    def get_every(self):
        return self._every

    def add_x(self, x):
        self._x_list.append(x)

    def clear_x_list(self):
        del self._x_list[:]

    def set_measures(self, measures_dic):
        for key, fn in measures_dic.items():
            self._functions[key] = fn
            self._values.setdefault(key, None)

    def get_measures(self):
        self._finish()
        return self._values

    def compute_measures(self):
        if not self._keep_iterates and self._session is not None:
            self._finish()
            for key, e in self._session.errors.items():
                # (a histogram / host measure that raised during the run: it
                # fails here, where the reference's observer would evaluate it)
                raise e
            return
        history = self._x_list
        for key, fn in self._functions.items():
            self._values[key] = np.fromiter((fn(x) for x in history),
                                            dtype=float, count=len(history))

    def get_observed_iterations(self):
        """Iteration indices the measure arrays stand for."""
        if not self._keep_iterates and self._session is not None:
            return list(self._session.points)
        return list(range(len(self._x_list)))

    def get_measure_classes(self):
        """{measure name: "board" | "ssim" | "histogram" | "host"} of the last
        device-mode run ({} before one)."""
        if self._session is None:
            return {}
        return dict(self._session.classes)

    # ---- used by the solvers (device mode) ----------------------------
    def _begin(self, n, iterations, refs=None):
        """Start of a device-mode run of a solver with n unknowns and
        `iterations` iterations: classify, upload, allocate the board.
        Returns the observation points.  refs: a dict that several observers of
        runs on the same data hand in (parameter_sweep.py), so that a reference
        they share is uploaded and summed once, not once per observer."""
        self._session = _DeviceRun(self._functions, n,
                                   observation_points(iterations, self._every),
                                   refs)
        for key in self._functions:
            self._values[key] = None
        return self._session.points

    def _observe(self, it, x, x_scale, layout=None):
        self._session.observe(it, x, x_scale, layout)

    def _finish(self):
        s = self._session
        if self._keep_iterates or s is None or s.done:
            return
        self._values.update(s.finish())


class _DeviceRun(object):
    """One device-mode run: the classified measures, the references on the
    device, the board and the values of the histogram and host classes."""

    def __init__(self, functions, n, points, refs=None):
        import torch
        from .device import device
        self.n = int(n)
        self.points = list(points)
        self.index = {p: k for k, p in enumerate(self.points)}
        self.done = False
        self.functions = functions
        self.descs, self.classes = {}, {}
        for key, fn in functions.items():
            d = probe_measure(fn, self.n)
            self.descs[key] = d
            self.classes[key] = classify(d)
        self._refs = {} if refs is None else refs     # id(ref) -> _Reference
        self.passes = self._plan()
        ssim = [k for k, c in self.classes.items() if c == "ssim"]
        self.ssim_slot = {k: 9 * len(self.passes) + j for j, k in enumerate(ssim)}
        width = 9 * len(self.passes) + len(ssim)
        self.board = None
        if width:
            self.board = torch.full((len(self.points), width), float("nan"),
                                    dtype=torch.float64, device=device())
        self.side = {k: np.full(len(self.points), np.nan)
                     for k, c in self.classes.items() if c in ("histogram", "host")}
        self._x0_dev = None
        self.errors = {}            # measure name -> first exception it raised

    def _ref(self, arr):
        r = self._refs.get(id(arr))
        if r is None:
            r = self._refs[id(arr)] = _Reference(arr)
        return r

    def _plan(self):
        """Passes of nsol_observe_*: each distinct reference of the pair
        measures and each distinct (gradient, gamma) of the prior measures
        needs one; they are paired up into as few passes as possible."""
        refs, grads, sq = [], [], False
        for key, c in self.classes.items():
            if c != "board":
                continue
            d = self.descs[key]
            if d.kind in PAIR_KINDS:
                r = self._ref(d.ref)
                if r not in refs:
                    refs.append(r)
            elif d.kind == "TK0":
                sq = True
            else:
                op, shape = d.grad[1], tuple(d.grad[2])
                gkey = (tuple(op.w), op.dimension, shape)
                gamma = d.gamma if d.kind == "Huber" else None
                if (gkey, gamma) not in [(g[0], g[2]) for g in grads]:
                    grads.append((gkey, shape, gamma))
        # a pass without a Huber term may carry any gamma: fold the gamma-free
        # entries into one of the same gradient that has a gamma
        kept = []
        for g in grads:
            if g[2] is None and any(h[0] == g[0] and h[2] is not None
                                    for h in grads):
                continue
            kept.append(g)
        m = max(len(refs), len(kept), 1 if sq else 0)
        passes = []
        for j in range(m):
            r = refs[j] if j < len(refs) else None
            g = kept[j] if j < len(kept) else None
            passes.append(dict(ref=r, grad=g, sq=(sq and j == 0)))
        # which pass serves which measure
        self.where = {}
        for key, c in self.classes.items():
            if c != "board":
                continue
            d = self.descs[key]
            for j, p in enumerate(passes):
                if d.kind in PAIR_KINDS:
                    ok = p["ref"] is self._ref(d.ref)
                elif d.kind == "TK0":
                    ok = p["sq"]
                else:
                    op = d.grad[1]
                    gkey = (tuple(op.w), op.dimension, tuple(d.grad[2]))
                    ok = p["grad"] is not None and p["grad"][0] == gkey and \
                        (d.kind != "Huber" or p["grad"][2] == d.gamma)
                if ok:
                    self.where[key] = j
                    break
        return passes

    # ------------------------------------------------------------------
    def observe(self, it, x, x_scale, layout):
        """Observation of iteration `it`: x the solver's unscaled device
        iterate (layout = (shape, pitch) when its rows are pitched), or a
        NumPy float64 array that is the iterate itself (get_x() before the
        first device iterate exists)."""
        from . import ops
        from .device import is_device_tensor, to_device
        k = self.index.get(it)
        if k is None:
            return
        if not is_device_tensor(x):
            if self._x0_dev is None:
                self._x0_dev = to_device(np.asarray(x, np.float64).reshape(-1),
                                         np.float64)
            x, x_scale, layout = self._x0_dev, 1.0, None
        shape, pitch = layout if layout is not None else ((x.numel(),), 0)
        for j, p in enumerate(self.passes):
            row = self.board[k, 9 * j:9 * j + 9]
            flags, kw = 0, {}
            vshape, vpitch, xv = shape, pitch, x
            if p["ref"] is not None:
                flags |= ops.OBS_PAIR
                kw["y"], kw["ybar"] = p["ref"].device(x.dtype), p["ref"].stats["mean"]
            if p["sq"]:
                flags |= ops.OBS_SQ
            if p["grad"] is not None:
                flags |= ops.OBS_GRAD
                gkey, gshape, gamma = p["grad"]
                kw["w"], kw["ndim"] = gkey[0], gkey[1]
                kw["gamma"] = 0.05 if gamma is None else gamma
                if gamma is not None:
                    flags |= ops.OBS_HUBER
                if pitch and tuple(gshape) != tuple(shape):
                    xv, vpitch = ops.from_pitched(x, shape, pitch), 0
                vshape = gshape
            ops.observe(xv, x_scale, row, vshape, pitch=vpitch, flags=flags, **kw)
        want_wide = any(c in ("ssim", "histogram") for c in self.classes.values())
        wide = ops.observe_widen(x, x_scale, shape, pitch) if want_wide else None
        for key, c in self.classes.items():
            d = self.descs[key]
            if c == "ssim":
                self._ssim(key, k, d, wide)
            elif c in ("histogram", "host") and key not in self.errors:
                # a measure that raises does not abort the solver's run: as with
                # keep_iterates=True, the error surfaces from compute_measures()
                try:
                    if c == "histogram":
                        self.side[key][k] = self._hist(d, wide)
                    else:
                        # (what Solver.get_x() returns: x * x_scale in the
                        # working dtype)
                        from .device import to_numpy
                        xc = ops.from_pitched(x, shape, pitch) if pitch else x
                        self.side[key][k] = self.functions[key](
                            to_numpy(ops.scale(xc, x_scale)))
                except Exception as e:      # noqa: BLE001 (re-raised later)
                    self.errors[key] = e

    @staticmethod
    def _f64():
        import torch
        return torch.float64

    def _ssim(self, key, k, d, wide):
        from . import ops
        from .similarity_measures import ssim_params
        r = self._ref(d.ref)
        win, C1, C2, cov_norm, count = ssim_params(
            d.shape, d.shape, np.float64, **d.ssim)
        slot = self.ssim_slot[key]
        ops.ssim_sum(wide, r.device(self._f64()), d.shape, win, C1, C2, cov_norm,
                     out=self.board[k, slot:slot + 1])

    def _hist(self, d, wide):
        from .similarity_measures import SimilarityMeasures, histogram_measure
        if d.kind == "Dice":
            return SimilarityMeasures.dice_score(wide.view(d.shape), d.ref)
        if d.kind == "entropy":
            return histogram_measure("entropy", wide, np.dtype(np.float64),
                                     bins=d.bins)
        r = self._ref(d.ref)
        return histogram_measure(d.kind, wide, np.dtype(np.float64), r.uploaded(),
                                 r.dtype, d.bins)

    def finish(self):
        """Reads the board (once) and turns every class into its values."""
        from .similarity_measures import ssim_params
        self.done = True
        b = self.board.cpu().numpy() if self.board is not None else None
        out = {}
        for key, c in self.classes.items():
            d = self.descs[key]
            if c == "board":
                j = self.where[key]
                ref = self._ref(d.ref).stats if d.kind in PAIR_KINDS else None
                out[key] = np.array([finalise(d.kind, b[k, 9 * j:9 * j + 9], ref)
                                     for k in range(len(self.points))])
            elif c == "ssim":
                count = ssim_params(d.shape, d.shape, np.float64, **d.ssim)[4]
                out[key] = b[:, self.ssim_slot[key]] / count
            else:
                out[key] = self.side[key]
        return out


class _Reference(object):
    """A reference array of the measures, on the device once per run: in the
    working dtype where that holds it exactly (float32 for a float32 run),
    otherwise in float64; plus its set-up constants."""

    def __init__(self, arr):
        self.arr = arr
        self._dev = {}
        self._up = None
        from . import ops
        self.dtype = ops.numpy_dtype(arr)
        self.stats = None           # set up with the first upload

    def _set_up(self, y):
        """Set-up constants from the first device copy (exact in any of its
        dtypes; the sums are float64)."""
        from . import ops
        st = ops.pair_stats(y, y)
        n = y.numel()
        ybar = st[7] / n
        css = ops.pair_stats(y, y, ybar, ybar)[2]
        self.stats = reference_stats(float(st[7]), float(st[5]), float(css), n)

    @staticmethod
    def _f64():
        import torch
        return torch.float64

    def device(self, dtype):
        """The reference as a flat contiguous device tensor that nsol_observe_*
        reads alongside x of `dtype`: dtype itself where exact, else float64."""
        import torch
        from .device import is_device_tensor, to_device
        if dtype in self._dev:
            return self._dev[dtype]
        a = self.arr
        t = None
        if dtype == torch.float32:
            if is_device_tensor(a):
                if a.dtype == torch.float32:
                    t = a.contiguous().view(-1)
            else:
                h = np.asarray(a).reshape(-1)
                if h.dtype == np.float32 or (h.dtype.kind in "fiub" and np.array_equal(
                        h.astype(np.float32).astype(np.float64),
                        h.astype(np.float64), equal_nan=False)):
                    t = to_device(h if h.dtype == np.float32 else
                                  h.astype(np.float32), np.float32)
        if t is None:
            if torch.float64 in self._dev:
                t = self._dev[torch.float64]
            elif is_device_tensor(a):
                t = a.contiguous().view(-1).to(torch.float64)
            else:
                t = to_device(np.asarray(a, dtype=np.float64).reshape(-1),
                              np.float64)
            self._dev[torch.float64] = t
        self._dev[dtype] = t
        if self.stats is None:
            self._set_up(t)
        return t

    def uploaded(self):
        """The reference as the histogram measures upload it (_upload)."""
        if self._up is None:
            from .similarity_measures import _upload
            self._up = _upload(self.arr)
        return self._up


add_accessors(Observer, ["name", "computational_time"])
add_accessors(Observer, ["x_list"], setters=False)
