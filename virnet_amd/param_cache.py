"""One cache for everything the library derives from a module's parameters: packed weight images, composed weights, pointer structs.

A module owns a ``ParamCache`` as an ordinary attribute made in ``__init__`` and asks it ``cache.get(slot, params, build)``.  ``slot`` is a
hashable name whose first element names the family -- ``("fwd", form)``, ``("dgrad", form)``, ``("thin",)``, ``("tail", form)``,
``("sft",)`` -- and all slots of a family are built from the same ``params``.  A leaf module: it imports nothing of the package."""


def param_key(params) -> tuple:
    """``(id(p), p.data_ptr(), p._version, p.device)`` of every parameter, None for None, end to end in one flat tuple: the one key of
    every derived value.  ``_version`` moves with an in-place write, ``data_ptr`` with ``p.data = ...`` / ``.to()``, ``id`` with a replaced
    Parameter object.  A write through ``.data`` moves none of them: the owner's ``invalidate()`` is for that."""
    key = ()
    for p in params:                                           # (the hit path of every launch: a loop beats a comprehension here)
        key += (None,) if p is None else (id(p), p.data_ptr(), p._version, p.device)
    return key


class ParamCache:
    """slot -> (key, value).  Copying or pickling a cache gives an EMPTY one: a copy's keys could never hit (they hold the original's
    storage pointers) and a ctypes struct of pointers cannot be pickled at all -- so ``copy.deepcopy(module)`` and ``torch.save(module)``
    carry no derived value and the original keeps its own."""

    def __init__(self):
        self._entries = {}

    def get(self, slot, params, build):
        """The slot's value, built by ``build()`` when the slot is empty or any of ``params`` moved since it was built.  A ``build()`` that
        returns None declines: nothing is stored or dropped.  On a miss the slot's siblings -- same family, hence same parameters -- that
        hold a stale key go too (images of an older parameter version); those with the current key stay (the range guard's fp32 re-run
        must not evict the split-fp16 image)."""
        key = param_key(params)
        hit = self._entries.get(slot)
        if hit is not None and hit[0] == key:
            return hit[1]
        value = build()
        if value is not None:
            self._entries = {s: h for s, h in self._entries.items() if s[0] != slot[0] or h[0] == key}
            self._entries[slot] = (key, value)
        return value

    def clear(self) -> None:
        self._entries = {}

    def slots(self) -> list:
        return list(self._entries)

    def __reduce__(self):
        return (ParamCache, ())
