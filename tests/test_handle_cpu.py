"""The handle base class of hpgfastq/engine.py over a stub in place of the C
library (no GPU): who calls <prefix>_close, and how often."""
import gc

import pytest

import hpgfastq.engine as E


class StubLib:
    """Every hpgq_* function: records (name, handle) and returns `rc[name]` (0).
    *_open writes a handle through its first argument."""

    def __init__(self, rc=None):
        self.calls = []
        self.rc = rc or {}

    def __getattr__(self, name):
        if not name.startswith("hpgq_"):
            raise AttributeError(name)

        def fn(first, *args):
            code = self.rc.get(name, 0)
            if name.endswith("_open"):
                self.calls.append((name, None))
                if code == 0:
                    first._obj.value = 0x1234
            else:
                self.calls.append((name, first.value))
            return code
        return fn

    def named(self, name):
        return [c for c in self.calls if c[0] == name]


HANDLES = [
    ("hpgq_kmers", lambda: E.Kmers(150)),
    ("hpgq_qdist", lambda: E.QualityDist(150)),
    ("hpgq_adapt", lambda: E.AdapterContent([b"ACGTACGTAC"])),
    ("hpgq_clip", lambda: E.AdapterClip([b"ACGTACGTAC"])),
    ("hpgq_ovl", lambda: E.OverlapClip()),
    ("hpgq_dup", lambda: E.Duplication()),
    ("hpgq_gs", lambda: E.Signature(4)),
    ("hpgq_parser", lambda: E.Parser()),
    ("hpgq_cgr", lambda: E.ChaosGame(4)),
]


@pytest.fixture
def stub(monkeypatch):
    s = StubLib()
    monkeypatch.setattr(E, "lib", s)
    return s


@pytest.mark.parametrize("prefix,make", HANDLES, ids=[p for p, _ in HANDLES])
def test_close_twice_calls_the_c_close_once(stub, prefix, make):
    h = make()
    assert stub.named(prefix + "_open") == [(prefix + "_open", None)]
    h.close()
    h.close()
    del h
    assert stub.named(prefix + "_close") == [(prefix + "_close", 0x1234)]


@pytest.mark.parametrize("prefix,make", HANDLES, ids=[p for p, _ in HANDLES])
def test_del_after_a_constructor_that_raised_calls_nothing(monkeypatch, prefix, make):
    s = StubLib(rc={prefix + "_open": -5})
    monkeypatch.setattr(E, "lib", s)
    with pytest.raises(E.HpgqError) as e:
        make()
    assert e.value.code == -5
    # the half-built object is gone (its __del__ ran when the exception let go of it)
    del e
    gc.collect()
    assert s.calls == [(prefix + "_open", None)]


def test_del_of_an_object_whose_init_never_ran_calls_nothing(stub):
    for cls in (E.Engine, E.Kmers, E.QualityDist, E.AdapterContent, E.AdapterClip, E.OverlapClip, E.Duplication, E.Signature,
                E.Parser, E.ChaosGame):
        h = cls.__new__(cls)
        h.close()
        h.__del__()
    with pytest.raises(TypeError):
        E.Engine("not params")   # raises before the handle exists
    assert stub.calls == []


@pytest.mark.parametrize("prefix,make", HANDLES, ids=[p for p, _ in HANDLES])
def test_the_context_manager_closes(stub, prefix, make):
    with make() as h:
        assert h._h and not stub.named(prefix + "_close")
    assert h._h is None
    assert stub.named(prefix + "_close") == [(prefix + "_close", 0x1234)]
    with pytest.raises(RuntimeError):
        with make() as h2:
            raise RuntimeError("body")
    assert h2._h is None and len(stub.named(prefix + "_close")) == 2


def test_pass_through_methods_call_the_prefixed_function_and_raise_its_code(monkeypatch):
    s = StubLib(rc={"hpgq_qdist_sync": -4})
    monkeypatch.setattr(E, "lib", s)
    with E.QualityDist(150) as q:
        q.reset()
        q.set_max_workgroups(1)
        q.reserve_length(300)
        q.count_device(E.device_batch(0, 0, 0, 0))
        with pytest.raises(E.HpgqError) as e:
            q.sync()
        assert e.value.code == -4 and "hpgq_qdist_sync" in str(e.value)
    assert [c[0] for c in s.calls] == ["hpgq_qdist_open", "hpgq_qdist_reset", "hpgq_qdist_debug_set_max_workgroups",
                                       "hpgq_qdist_reserve_length", "hpgq_qdist_count_device", "hpgq_qdist_sync",
                                       "hpgq_qdist_close"]
