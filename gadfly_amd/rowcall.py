"""
The host side the one-wave batch calls share (``gf_loglike_grad``, ``gf_solve_batch``, ``gf_var_batch``,
``gf_predict_batch_at``): the check of a stacked coefficient pack, the split of a batch
into groups under a byte cap, the query axes, and the loop that launches one group after the other
(:class:`GroupedCall`).  A problem's result does not depend on the group it lands in.
"""
import numpy as np
import torch

from . import _lib


def check_pack_batch(B, Jr, Jc, real, comp, diag_add):
    """ValueError unless a stacked coefficient pack holds exactly B problems of the structure (Jr, Jc) in the
    layout the device reads (real (2, B, max(Jr, 1)), comp (4, B, max(Jc, 1)), diag_add (B,)): gf_loglike_grad
    indexes every array by the problem, so a shorter pack must never reach it."""
    want = ((2, B, max(Jr, 1)), (4, B, max(Jc, 1)), (B,))
    got = tuple(tuple(np.shape(x)) for x in (real, comp, diag_add))
    if got != want:
        raise ValueError(f"coefficient pack of shapes {got} does not match the batch of {B} problems "
                         f"(expected {want})")


def group_plan(per, B, cap_bytes, nothing):
    """(doubles per problem, problems per group, number of groups) of B problems of ``per`` workspace doubles each
    under a cap of ``cap_bytes`` per group (one problem at least); ValueError(``nothing``) when the library gave no
    size (``per`` <= 0)."""
    per = int(per)
    if per <= 0:
        raise ValueError(nothing)
    group = int(max(1, min(B, int(cap_bytes) // (8 * per))))
    return per, group, (B + group - 1) // group


def check_query_axes(B, N, shape, nobs=None, nq=None, empty_ok=False):
    """The query axes of B problems of N rows, on the host: ``shape`` of the stamps -- (M,) or (1, M) shared, (B, M),
    or None for no queries -- and the (B,) counts of real observed rows (<= N) and real queries (<= M), or None.
    Returns (M, nobs, nq), the counts as contiguous int64 arrays.  M = 0 is an error unless ``empty_ok``."""
    M = 0
    if shape is not None:
        shape = tuple(shape)
        if len(shape) == 1:
            shape = (1,) + shape
        if len(shape) != 2 or shape[0] not in (1, B) or (shape[1] < 1 and not empty_ok):
            raise ValueError(f"query times of shape {shape} for a batch of {B} problems")
        M = int(shape[1])
    counts = []
    for cnt, full in ((nobs, N), (nq, M)):
        if cnt is not None:
            cnt = np.ascontiguousarray(cnt, dtype=np.int64)
            if cnt.shape != (B,) or np.any(cnt < 0) or np.any(cnt > full):
                raise ValueError("dimension mismatch")
        counts.append(cnt)
    return M, counts[0], counts[1]


def query_axes(engine, ts, nobs=None, nq=None, empty_ok=False):
    """:func:`check_query_axes`, then the upload: (stamps as a contiguous float64 device tensor (1 or B, M) -- None
    without queries --, M, nobs, nq as int64 device tensors or None).  ``ts``: a host array or a device tensor; None
    stands for no queries where ``empty_ok``."""
    dev = engine.device
    if ts is not None or not empty_ok:
        ts = torch.as_tensor(ts, dtype=torch.float64).to(dev)
    M, nobs, nq = check_query_axes(engine.B, engine.N, None if ts is None else ts.shape, nobs, nq, empty_ok)
    ts = (ts[None, :] if ts.ndim == 1 else ts).contiguous() if M else None
    nobs, nq = (None if c is None else torch.as_tensor(c, dtype=torch.int64, device=dev) for c in (nobs, nq))
    return ts, M, nobs, nq


class GroupedCall:
    """One C entry point launched group by group over an engine's data (t, y - mean, diag on the device).

    ``plan``: the ``(per, group, ngroups)`` of :func:`group_plan`; the workspace of one group is allocated here.
    ``packs``: stacked host coefficient packs ``(real, comp[, diag_add])`` of all B problems, or None.  :meth:`run`
    calls ``call(self)`` once per group with the group in these attributes:

    * ``nb``, ``b0``: problems in the group, the first one's index;
    * ``coef``: per pack the device pointers of the group's slice of it, uploaded -- a_r, c_r, a_c, b_c, c_c, d_c and,
      where the pack has one, diag_add; six null pointers for a pack that is None;
    * ``data``: ``(t, tbs, diag, dbs, y, ybs)``, pointers at the group's first problem and batch strides;
    * ``work``: ``(pointer, doubles per problem)`` of the workspace; ``stream``: the current stream's handle;
      ``y=``: a float64 device tensor (1 or B, N) that stands in for the engine's y (the residuals of a linear mean
      model, :mod:`gadfly_amd.linmodel`); None: the engine's own;
    * :meth:`at`, the pointer of any other per-problem tensor at the group's first problem;
    * :meth:`launch`, the C call itself between a pair of HIP events, its status checked.
    """

    def __init__(self, engine, name, plan, *packs, y=None):
        self.name, self.fn = name, getattr(engine.lib, name)
        if y is not None and (y.ndim != 2 or y.shape[0] not in (1, engine.B) or y.shape[1] != engine.N
                              or y.dtype != torch.float64 or not y.is_contiguous()):
            raise ValueError(f"data of shape {tuple(y.shape)} for a batch of {engine.B} problems of {engine.N} rows")
        self.y = y
        self.engine, self.B = engine, engine.B
        self.per, self.group, self.ngroups = plan
        self._f64 = dict(dtype=torch.float64, device=engine.device)
        self.stream = torch.cuda.current_stream(engine.device).cuda_stream
        self._work = torch.empty((self.group * self.per,), **self._f64)
        self.work = (self._work.data_ptr(), self.per)
        self.packs = [None if pk is None else [np.ascontiguousarray(x, dtype=np.float64) for x in pk]
                      for pk in packs]
        self.events = []

    @property
    def plan(self):
        """The plan as the result dicts hold it."""
        return dict(workspace_bytes=8 * self.per * self.group, groups=self.ngroups, group_size=self.group)

    def at(self, x, per=1):
        """Pointer of the group's first problem in a tensor of ``per`` elements per problem (None -> NULL)."""
        return None if x is None else x.data_ptr() + x.element_size() * self.b0 * per

    def _upload(self, pack):
        """The group's slice of a stacked host pack on the device -> (the tensors, their pointers)."""
        if pack is None:
            return (), [None] * 6
        b = slice(self.b0, self.b0 + self.nb)
        dev = [torch.as_tensor(np.ascontiguousarray(x[:, b] if x.ndim == 3 else x[b]), **self._f64) for x in pack]
        return dev, [row.data_ptr() for x in dev[:2] for row in x] + [x.data_ptr() for x in dev[2:]]

    def launch(self, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(self.fn(*args), self.name)
        e1.record()
        self.events.append((e0, e1))

    def run(self, call, only=None):
        """``call(self)`` for each group in turn -- ``only``: for the groups of these indices --; returns the pairs
        of HIP events around the launches."""
        eng = self.engine
        t, y, dg = eng.t, eng.y if self.y is None else self.y, eng.diag
        tbs, ybs = eng._bs(t), eng._bs(y)
        dbs = 0 if dg is None else eng._bs(dg)
        only = None if only is None else {int(i) for i in only}
        for b0 in range(0, self.B, self.group):
            if only is not None and b0 // self.group not in only:
                continue
            self.b0, self.nb = b0, min(self.group, self.B - b0)
            # (the uploaded slices are held until the next group's replace them: the launch is enqueued by then)
            self._held, self.coef = zip(*[self._upload(pk) for pk in self.packs])
            self.data = (self.at(t, tbs), tbs, self.at(dg, dbs), dbs, self.at(y, ybs), ybs)
            call(self)
        return self.events
