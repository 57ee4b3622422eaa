"""CPU tests of smallround.ResultBlocks, the one owner of "may this result block be written again":
a block is leased as a fresh ndarray that is the base of the model's arrays, and is free again only
once nothing reaches that lease — whatever the caller made of the model. Pageable memory stands in
for the pinned blocks (the allocator argument)."""
import gc

import numpy as np
import pytest
import torch

from fedn_amd.layout import Layout
from fedn_amd.smallround import _POOL, ResultBlocks
from model_holders import HOLDERS, held_bytes

_fastpack = pytest.importorskip("fedn_amd._fastpack")

LAYOUTS = {"mnist": [(64, 784), (64,), (32, 64), (32,), (10, 32), (10,)],      # 210,688 B
           "minimum": [(0,), (64,), (0, 5), (10,)]}
pytestmark = pytest.mark.parametrize("shapes", list(LAYOUTS.values()), ids=list(LAYOUTS))


def _pageable(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8)


class _Models:
    """Models leased the way a small round does it: the lease is kept by the model's arrays alone."""

    def __init__(self, shapes):
        self.lay = Layout.of([np.zeros(s, np.float32) for s in shapes])
        offs = {i: off for i, off, _ in self.lay.pack_plan}
        self.plan = _fastpack.plan([(tuple(sh), np.dtype(dt), offs.get(i, 0))
                                    for i, (sh, dt) in enumerate(zip(self.lay.shapes, self.lay.dtypes))])
        self.blocks = ResultBlocks(_pageable)
        self.rounds = 0

    def round(self):
        """A model whose every byte is this round's number (1, 2, ...), and its block's address."""
        lease = self.blocks.lease(self.lay.nbytes)
        self.rounds += 1
        lease[:] = self.rounds
        return _fastpack.views(self.plan, lease), lease.ctypes.data

    def pooled(self):
        return len(self.blocks._pools[self.lay.nbytes])

    def free_addresses(self):
        """The addresses of ``_POOL`` models held at once: every free pooled block is among them."""
        live = [self.round() for _ in range(_POOL)]
        return [addr for _, addr in live]


def test_a_lease_is_the_block_and_the_base_of_its_views(shapes):
    m = _Models(shapes)
    lease = m.blocks.lease(m.lay.nbytes)
    assert lease.dtype == np.uint8 and lease.shape == (m.lay.nbytes,)
    assert lease.flags.c_contiguous and lease.flags.writeable
    assert not isinstance(lease.base, np.ndarray)      # numpy would point the views past the lease at it
    (ent,) = m.blocks._pools[m.lay.nbytes]
    assert lease.ctypes.data == ent[0].data_ptr()
    views = _fastpack.views(m.plan, lease)
    assert all(v.base is lease for v in views)
    views[1][...] = 2.5
    off = views[1].ctypes.data - lease.ctypes.data
    assert lease[off:off + views[1].nbytes].view(np.float32).tolist() == [2.5] * views[1].size
    assert views[1][3:7].base is lease and views[1].view(np.uint8).base is lease


def test_held_models_keep_their_blocks_and_dropped_ones_return_them(shapes):
    m = _Models(shapes)
    held = [m.round() for _ in range(3 * _POOL)]
    assert len({addr for _, addr in held}) == len(held)          # no two live models share a block
    assert m.pooled() == _POOL                                   # the blocks beyond are not kept
    for r, (model, _) in enumerate(held, 1):                     # every model as its round wrote it
        assert all((a.view(np.uint8) == r).all() for a in model)
    seen = {addr for _, addr in held}
    del held, model
    assert m.round()[1] in seen and m.pooled() == _POOL


@pytest.mark.parametrize("kind", list(HOLDERS))
def test_whatever_holds_a_model_holds_its_block(kind, shapes):
    m = _Models(shapes)
    model, addr = m.round()
    holder = HOLDERS[kind](model)
    want = held_bytes(holder)
    assert want.size and (want == 1).all()
    del model
    for _ in range(2):
        assert addr not in m.free_addresses()                    # each of these rounds writes its block
    assert np.array_equal(held_bytes(holder), want)
    del holder
    assert addr in m.free_addresses()


def test_a_model_in_a_reference_cycle_holds_its_block_until_collected(shapes):
    m = _Models(shapes)
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        model, addr = m.round()
        cycle = [model]
        cycle.append(cycle)
        del model, cycle
        assert addr not in m.free_addresses()
        gc.collect()
        assert addr in m.free_addresses()
    finally:
        if was_enabled:
            gc.enable()
