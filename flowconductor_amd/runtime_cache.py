"""The one place where modules keep run-time state derived from their parameters.

Layers cache kernel-layout copies of their weights (pre-masked, zero-padded, folded matrices), ``DevicePack`` plans with
raw device pointers, index tensors and memoised fast-path predicates.  None of it is model state.  All of it lives in one
``Store`` per module, at ``module.__dict__["_fc_cache"]``, written through ``memo`` (and its wrappers ``static_memo`` and
``device_plan``).  A ``Store`` copies and pickles as an EMPTY store, so ``copy.deepcopy``, ``pickle`` and
``torch.save(module)`` carry parameters and buffers only and a copy starts cold and re-packs from ITS OWN parameters --
for any ``nn.Module``, with nothing to list and nothing to inherit from.

Weight images are keyed with ``cache_key``: the parameters' version counters and storage pointers.  In-place writes THROUGH
``.data`` (``p.data.copy_(ema)``, ``p.data.clamp_()``, some checkpoint loaders) change neither; ``invalidate_hip_caches()``
bumps an epoch that is part of every such key.  ``nn.Module.train()`` of this package's modules calls it, so a cache never
survives a switch into or out of training mode; after ``.data`` surgery on an eval-mode model call it yourself.
"""
from flowconductor_amd import options


class Store(dict):
    """``{slot: (key, value)}``.  Copies and pickles of it are empty (``fc_pack_job`` structs carry raw device pointers and
    cannot be pickled at all)."""

    def __deepcopy__(self, memo):
        return type(self)()

    def __reduce_ex__(self, protocol):
        return type(self), ()


def _store(owner):
    store = owner.__dict__.get("_fc_cache")
    if store is None:
        store = owner.__dict__["_fc_cache"] = Store()       # (not through nn.Module.__setattr__)
    return store


def memo(owner, slot, key, compute):
    """The value ``owner`` keeps under ``slot`` if it was stored for an equal ``key``; otherwise ``compute()``, stored for
    ``key``.  The key is compared as given: what must invalidate the entry (``cache_key`` of the tensors it was made from,
    a device, a width) is the caller's to put in."""
    store = owner.__dict__.get("_fc_cache")
    if store is None:
        store = _store(owner)
    entry = store.get(slot)
    if entry is None or entry[0] != key:
        entry = store[slot] = (key, compute())
    return entry[1]


def cached(owner, slot):
    """What ``owner`` holds under ``slot`` right now (None when nothing); computes nothing."""
    entry = owner.__dict__.get("_fc_cache", {}).get(slot)
    return None if entry is None else entry[1]


_cache_epoch = 0


def invalidate_hip_caches():
    """Drop every packed-weight cache of this package (re-packed on the next call that needs them)."""
    global _cache_epoch
    _cache_epoch += 1


_paranoid_tick = 0


def cache_key(*tensors, extra=()):
    """Key of a packed copy of ``tensors``: version counter, storage pointer and device of each + the epoch.  With
    ``options.paranoid_caches`` no two keys are equal: every lookup misses and re-packs."""
    global _paranoid_tick
    if options.get("paranoid_caches"):
        _paranoid_tick += 1
        return (("paranoid", _paranoid_tick),) + (_cache_epoch,) + tuple(extra)
    return tuple((t._version, t.data_ptr(), t.device) for t in tensors) + (_cache_epoch,) + tuple(extra)


def static_memo(module, slot, key, compute):
    """``memo`` for as long as ``key`` and the cache epoch stand -- for the parts of a fast-path predicate that only depend on
    how the module is built (layer types, widths, activations, training flag): re-deriving them on every call was a fifth
    of the host time of a small batch."""
    return memo(module, slot, (_cache_epoch,) + tuple(key), compute)


def device_plan(owner, slot, where, build):
    """The device pack plan ``(pack, packed, ...)`` = ``build()`` that ``owner`` keeps under ``slot``.  Its jobs hold raw
    device pointers, so it is rebuilt whenever ``where`` -- the storages it reads and whatever else it was built around --
    differs from the one it was built for, and for nothing else: the cache epoch reaches it through ``DevicePack.refresh``.
    An object that ``where`` names by ``id()`` must be returned by ``build()`` into the tail of the plan, so that the id
    cannot be reused while the plan lives.  The caller refreshes ``plan[0]``."""
    return memo(owner, slot, where, build)


def param_list(module):
    """``tuple(module.parameters())`` memoised on the module (walking the module tree on every call is a third of the
    per-layer host time of a small batch) together with WHERE each parameter hangs: the memo is valid only while every slot
    still holds the same Parameter object (``lin.weight = nn.Parameter(...)``, ``load_state_dict(assign=True)`` and late
    parametrizations replace objects without touching versions or pointers of the orphans) and the cache epoch stands;
    modules drop it in ``_apply`` (.to / .cuda / .float) with ``drop_param_list``."""
    store = _store(module)
    entry = store.get("param_list")
    if entry is None or entry[0] != _cache_epoch or not all(m._parameters.get(n) is p for m, n, p in entry[2]):
        slots = tuple((m, n, p) for m in module.modules() for n, p in m._parameters.items() if p is not None)
        entry = store["param_list"] = (_cache_epoch, tuple(module.parameters()), slots)
    return entry[1]


def drop_param_list(module):
    module.__dict__.get("_fc_cache", {}).pop("param_list", None)


def buffer_list(module):
    """The buffers of ``module`` and its sub-modules (power-method vectors, running statistics), memoised like
    ``param_list``: valid while the cache epoch stands and every slot still holds the same tensor."""
    store = _store(module)
    entry = store.get("buffer_list")
    if entry is None or entry[0] != _cache_epoch or not all(m._buffers.get(n) is t for m, n, t in entry[2]):
        slots = tuple((m, n, t) for m in module.modules() for n, t in m._buffers.items() if t is not None)
        entry = store["buffer_list"] = (_cache_epoch, tuple(t for _, _, t in slots), slots)
    return entry[1]


def module_list(module):
    """``tuple(module.modules())``, kept on the module and rebuilt when the cache epoch moves or a child is added /
    removed: walking ``modules()`` on every call was the largest single item of the per-layer host time."""
    store = _store(module)
    entry = store.get("module_list")
    key = (_cache_epoch, len(module._modules))
    if entry is None or entry[0] != key:
        entry = store["module_list"] = (key, tuple(module.modules()))
    return entry[1]


def has_hooks(module):
    """True when ``module`` or a sub-module carries forward (pre-)hooks (old-style weight_norm refreshes ``weight``
    in one): the fast paths read the weights directly and never go through ``__call__``, so they step aside."""
    return any(m._forward_hooks or m._forward_pre_hooks for m in module_list(module))


def structure_key(net):
    """The cheap MUTABLE inputs of a conditioner's fast-path predicate, for ``static_memo`` keys: per residual block the
    identity of its activation, its dropout probability and its own training flag (``block.train()`` / a swapped
    activation / ``dropout.p = 0.1`` after the first call must re-derive the predicate)."""
    blocks = getattr(net, "blocks", ())
    return (net.training, id(getattr(net, "activation", None))) + tuple(
        (id(getattr(b, "activation", None)), getattr(getattr(b, "dropout", None), "p", 0.0), b.training) for b in blocks)
