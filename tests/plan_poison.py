"""Instrument for engine.Pool: every buffer the pool has back holds NaN until its next owner writes it.

engine.Pool is a best-fit free list; the plan builders call pool.get / pool.put by hand.  The contract -- a buffer is put only after
the plan.add of its last reader -- is enforced by nothing, and a put that sits one line too early is invisible unless best fit hands
that buffer to a layer planned in between, which depends on the shape.  `poisoned_pool()` makes the check independent of the shape.
For its duration it patches three attributes (plus engine.padded_input for one assertion, see the limits; all restored on exit, no file
outside tests/ changes):

 * engine.Plan.__init__  the new plan's pool gets a back-reference to the plan, a dict of the buffers currently out and the set of
                         flats it has handed out so far;
 * engine.Pool.get       calls the original; a flat that is already out raises AssertionError (the free list held it twice); a flat
                         seen for the first time is filled with NaN right away, at build time -- eagerly, NOT as a plan step, because
                         _run_fpn, _run_head and MNBlock.forward stage their inputs into freshly got buffers outside the plan before
                         plan.run();
 * engine.Pool.put       a flat that is not out raises AssertionError (a double put, or a buffer of another pool); otherwise a plan
                         step `flat.fill_(nan)` over the WHOLE flat (not only the [:need] view) is appended and the original called.
                         From the release point in stream order until the next owner writes it the buffer holds NaN on every run,
                         whether or not this shape happens to reuse it.

With workspaces=True the torch.empty workspaces are poisoned too: ops.groupnorm_workspace, ops.se_workspace and ops.mbconv_pool_buffer
return NaN-filled tensors, ops.sk_workspace has everything behind its zeroed 2048-float header filled with NaN.  A kernel whose first
use of such a workspace depends on its content then computes NaN.

The criterion the tests apply is bit equality of the plan's outputs with the uninstrumented plan's (same commit, same kernels, same
order), not a NaN scan: a ReLU or max-pool epilogue turns a poisoned operand into a clean-looking zero.

Limits:
 * An instrumented plan has extra steps (named POISON_STEP), so step_flops / step_info indices and mark ranges of an instrumented
   plan are not meaningful: nothing may read them for their meaning (a mark still is a valid index range of plan.steps, which is all
   TwoLanePipeline needs).
 * A buffer that is staged from outside the plan must be a fresh flat (its NaN fill is eager); a reused one would have its poison
   step run inside plan.run(), after the staging.  True at all three sites today; `Session.still_out` reports `fresh` per buffer
   and engine.padded_input is wrapped to assert it, the tests assert it for _run_head's pyramid and MNBlock's input.
 * Buffers that are allocated with torch.empty directly in engine.py and parked in plan.keep (_gn_coef, the post-processing scratch
   of add_postprocess) never pass through the pool: the instrument does not see them.
"""
import contextlib
from collections import namedtuple

import torch

from pytorch_object_detection_amd import engine, ops

NAN = float("nan")
POISON_STEP = "pool.poison"
SK_HEADER = 2048          # floats: the flag header of ops.sk_workspace, zero before and after every launch

Out = namedtuple("Out", "rows C fresh flat")     # a buffer that is out: the (rows, C) it was got for, whether the flat was new then


class Session:
    """What poisoned_pool() yields: the plans built under it, and the queries the tests make after a build."""

    def __init__(self):
        self.plans = []

    @staticmethod
    def still_out(plan):
        """The buffers got from plan.pool and not put back, in the order they were got."""
        return list(plan.pool._out.values())

    @staticmethod
    def out_shapes(plan):
        return sorted((o.rows, o.C) for o in plan.pool._out.values())

    @staticmethod
    def free_duplicates(plan):
        """Flats that sit on the free list more than once (each would be handed to two owners)."""
        ids = [id(t) for t in plan.pool.free]
        return sorted({i for i in ids if ids.count(i) > 1})

    @staticmethod
    def total(plan):
        return plan.pool.total

    @staticmethod
    def poison_steps(plan):
        return sum(1 for n in plan.names if n == POISON_STEP)


def _arm(pool, plan):
    pool._plan, pool._out, pool._seen = plan, {}, {}


@contextlib.contextmanager
def poisoned_pool(workspaces=True):
    session = Session()
    Plan, Pool = engine.Plan, engine.Pool
    saved = [(Plan, "__init__", Plan.__init__), (Pool, "get", Pool.get), (Pool, "put", Pool.put), (engine, "padded_input", engine.padded_input)]
    plan_init, pool_get, pool_put, padded_input = (s[2] for s in saved)

    def init(self, *args, **kwargs):
        plan_init(self, *args, **kwargs)
        _arm(self.pool, self)
        session.plans.append(self)

    def get(self, rows, C):
        r = pool_get(self, rows, C)
        if not hasattr(self, "_out"):        # a Pool made on its own, or by a Plan built before the instrument was active: checks only
            _arm(self, None)
        flat = r._flat
        if id(flat) in self._out:
            raise AssertionError(f"pool.get({rows}, {C}): the flat handed out is already out as {self._out[id(flat)][:2]} -- it was on the free list twice")
        fresh = id(flat) not in self._seen
        if fresh:
            self._seen[id(flat)] = flat      # (the reference keeps the id from being recycled)
            flat.fill_(NAN)
        self._out[id(flat)] = Out(rows, C, fresh, flat)
        return r

    def put(self, r):
        flat = getattr(r, "_flat", None)
        if flat is None or id(flat) not in getattr(self, "_out", {}):
            raise AssertionError("pool.put: this buffer is not out of this pool (a second put of it, or a buffer of another pool)")
        del self._out[id(flat)]
        if self._plan is not None:
            self._plan.add(POISON_STEP, lambda f=flat: f.fill_(NAN))
        pool_put(self, r)

    def padded(plan, rows, C):
        full, view = padded_input(plan, rows, C)
        flat = getattr(full, "_flat", None)
        if flat is not None:
            assert plan.pool._out[id(flat)].fresh, "padded_input: a staging buffer must be a fresh flat (its poison would run after the copy-in)"
        return full, view

    patches = [(Plan, "__init__", init), (Pool, "get", get), (Pool, "put", put), (engine, "padded_input", padded)]
    if workspaces:
        def nan_ws(fn):
            def wrapped(*args, **kwargs):
                return fn(*args, **kwargs).fill_(NAN)
            return wrapped

        gn_ws, se_ws, mb_buf, sk_ws = ops.groupnorm_workspace, ops.se_workspace, ops.mbconv_pool_buffer, ops.sk_workspace

        def mbconv_pool_buffer(*args, **kwargs):
            buf, ntile = mb_buf(*args, **kwargs)
            return buf.fill_(NAN), ntile

        def sk_workspace(*args, **kwargs):
            ws = sk_ws(*args, **kwargs)
            ws[SK_HEADER:].fill_(NAN)
            return ws

        saved += [(ops, "groupnorm_workspace", gn_ws), (ops, "se_workspace", se_ws), (ops, "mbconv_pool_buffer", mb_buf), (ops, "sk_workspace", sk_ws)]
        patches += [(ops, "groupnorm_workspace", nan_ws(gn_ws)), (ops, "se_workspace", nan_ws(se_ws)), (ops, "mbconv_pool_buffer", mbconv_pool_buffer),
                    (ops, "sk_workspace", sk_workspace)]
    try:
        for obj, name, fn in patches:
            setattr(obj, name, fn)
        yield session
    finally:
        for obj, name, fn in saved:
            setattr(obj, name, fn)
