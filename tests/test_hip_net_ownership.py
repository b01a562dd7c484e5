"""Who owns what in hipnet.dec_ipt: a native net stores raw pointers into one packed weight set (cfen_net_set_param copies nothing), so a net
must not outlive the set it was built on, must be destroyed exactly once, and a healthy compute-type flip must neither repack nor rebuild.

No GPU: cfen_net_create / cfen_net_set_param / cfen_net_destroy are host-only (tests/test_cabi.py relies on the same), so the real dec_ipt runs
on CPU tensors and `_net_for` builds real handles.  Creates and destroys are observed by wrapping the loaded library's entry points; a handle is
identified by its creation number, never by its address (the allocator may hand a destroyed net's address to the next one)."""
import gc

import pytest
import torch

from cfen_vit_dehazing_amd import _lib
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.hipnet import dec_ipt
from cfen_vit_dehazing_amd.manifest import generate_state_dict

CFG = NetConfig(8, 2, patch_size=8, load_size=64)
B = 2
CPU = torch.device("cpu")
_SD = {}


def state_dict(mode):
    if mode not in _SD:
        _SD[mode] = generate_state_dict(CFG, mode=mode)
    return _SD[mode]


class Handles:
    """creation number (1, 2, ...) of every native net, the parameter pointers it was given, and the order in which they were destroyed"""

    def __init__(self, lib, monkeypatch):
        self.created = 0
        self.live = {}              # address -> creation number
        self.destroyed = []         # creation numbers, in order
        self.stray = []             # addresses destroyed while not live (a second destroy): recorded, NOT passed on to the library
        self.params = {}            # creation number -> {name: device pointer}
        create, destroy, set_param = lib.cfen_net_create, lib.cfen_net_destroy, lib.cfen_net_set_param

        def on_create(hp, cc):
            rc = create(hp, cc)
            if rc == 0:
                self.created += 1
                self.live[hp._obj.value] = self.created
                self.params[self.created] = {}
            return rc

        def on_destroy(h):
            if h.value not in self.live:
                self.stray.append(h.value)
                return
            self.destroyed.append(self.live.pop(h.value))
            destroy(h)

        def on_set_param(h, name, p, nbytes):
            self.params[self.live[h.value]][name.decode()] = p.value
            return set_param(h, name, p, nbytes)

        monkeypatch.setattr(lib, "cfen_net_create", on_create)
        monkeypatch.setattr(lib, "cfen_net_destroy", on_destroy)
        monkeypatch.setattr(lib, "cfen_net_set_param", on_set_param)

    def number(self, rec):
        return self.live[rec.handle.value]


@pytest.fixture
def handles(monkeypatch):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # packing on the CPU is thousands of tiny tensor ops: a thread team per op costs far more than it saves
    yield Handles(_lib.load(), monkeypatch)
    torch.set_num_threads(threads)


def make(mode, dtype):
    net = dec_ipt(CFG, compute_dtype=dtype)
    net.load_state_dict(state_dict(mode), strict=True)
    return net


def pointers(pset):
    return {name: t.data_ptr() for name, t in pset.packed.items()}


def every_live_net_points_into_the_set_in_force(net, handles):
    """the handles alive in the library are exactly the records of the module's sets, each filed under its own compute type, and every parameter
    pointer a handle was given is the address of that tensor in the set now in force for the type"""
    recs = {handles.number(r): (dt, r) for dt, s in net._sets.items() for r in s.nets.values()}
    assert sorted(recs) == sorted(handles.live.values())
    for n, (dt, r) in recs.items():
        assert r.key.dtype == dt == net._sets[dt].dtype
        assert handles.params[n] == pointers(net._sets[dt])


def two_types_alive(handles):
    net = make("trained", "fp16")
    net._net_for(B, CPU)
    net.set_compute_dtype("fp32")
    net._net_for(B, CPU)
    assert handles.created == 2 and handles.destroyed == []
    return net


def test_a_net_dies_with_the_pending_set_it_points_into(handles):
    """a packed set with uninitialised ActNorm layers is dropped, not cached, when the compute type changes (set_compute_dtype): the nets built on it
    go with it, and the way back repacks and builds a new handle on the new memory"""
    net = make("reference_init", "fp16")
    net._net_for(B, CPU)
    assert handles.created == 1
    net.set_compute_dtype("fp32")
    assert handles.destroyed == [1], "the fp16 net outlived the packed set its pointers refer to"
    assert net.actnorm_pending()
    net._net_for(B, CPU)
    net.set_compute_dtype("fp16")
    assert handles.destroyed == [1, 2]              # (the fp32 set is pending as well)
    c = net._net_for(B, CPU)
    assert handles.number(c) == 3 and handles.created == 3
    assert net._net_for(B, CPU) is c
    every_live_net_points_into_the_set_in_force(net, handles)
    assert handles.stray == []


def test_a_healthy_flip_neither_repacks_nor_rebuilds(handles):
    """initialised ActNorm: both types' packed sets and nets stay resident across set_compute_dtype (what the per-type cache is for)"""
    net = make("trained", "fp16")
    a = net._net_for(B, CPU)
    assert not net.actnorm_pending()
    p16 = pointers(net._sets[torch.float16])
    net.set_compute_dtype("fp32")
    b = net._net_for(B, CPU)
    p32 = pointers(net._sets[torch.float32])
    net.set_compute_dtype("fp16")
    assert net._net_for(B, CPU) is a and pointers(net._ensure_packed(CPU)) == p16
    net.set_compute_dtype("fp32")
    assert net._net_for(B, CPU) is b and pointers(net._ensure_packed(CPU)) == p32
    assert handles.created == 2 and handles.destroyed == [] and handles.stray == []
    every_live_net_points_into_the_set_in_force(net, handles)


@pytest.mark.parametrize("how", ["invalidate", "load_state_dict", "float"])
def test_dropping_the_weights_destroys_every_net_exactly_once(handles, how):
    net = two_types_alive(handles)
    if how == "invalidate":
        net.invalidate()
    elif how == "load_state_dict":
        net.load_state_dict(state_dict("trained"), strict=True)
    else:
        net.float()                                 # (through nn.Module._apply)
    assert sorted(handles.destroyed) == [1, 2] and handles.live == {} and net._sets == {}
    del net
    gc.collect()
    assert sorted(handles.destroyed) == [1, 2] and handles.stray == []


def test_release_other_dtypes_keeps_the_current_type_only(handles):
    net = two_types_alive(handles)
    kept = net._net_for(B, CPU)
    net.release_other_dtypes()
    assert list(net._sets) == [torch.float32] and net._live_nets() == [kept]
    assert handles.destroyed == [1] and handles.number(kept) == 2
    every_live_net_points_into_the_set_in_force(net, handles)
    del net, kept
    gc.collect()
    assert handles.destroyed == [1, 2] and handles.stray == []


def test_every_net_is_destroyed_when_the_module_is_collected(handles):
    net = two_types_alive(handles)
    net._net_for(B + 1, CPU)
    net._free_nets()                                # nets go, packed sets stay: the next net is built on the same tensors
    assert sorted(handles.destroyed) == [1, 2, 3] and set(net._sets) == {torch.float16, torch.float32}
    net._net_for(B, CPU)
    every_live_net_points_into_the_set_in_force(net, handles)
    del net
    gc.collect()
    assert handles.created == 4 and sorted(handles.destroyed) == [1, 2, 3, 4] and handles.live == {} and handles.stray == []
