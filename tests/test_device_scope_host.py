"""_lib.DeviceScope without a device and without the library: `keep` takes anything that has a free()."""
import pytest

from graph_kmer_index_amd import _lib


class Fake:
    def __init__(self, name, log, fails=False):
        self.name, self.log, self.fails, self.freed = name, log, fails, 0

    def free(self):
        self.freed += 1
        if self.freed == 1:
            self.log.append(self.name)
        if self.fails:
            raise RuntimeError("free of %s" % self.name)


def test_everything_kept_is_freed_on_normal_exit_last_made_first():
    log = []
    with _lib.DeviceScope() as s:
        a, b, c = (s.keep(Fake(n, log)) for n in "abc")
        assert isinstance(a, Fake) and log == []
    assert log == ["c", "b", "a"]
    assert (a.freed, b.freed, c.freed) == (1, 1, 1)


def test_everything_kept_is_freed_on_an_exception_and_it_propagates():
    log = []
    with pytest.raises(KeyError, match="boom"):
        with _lib.DeviceScope() as s:
            s.keep(Fake("a", log))
            s.keep(Fake("b", log))
            raise KeyError("boom")
    assert log == ["b", "a"]


def test_a_released_object_is_returned_and_not_freed():
    log = []
    with _lib.DeviceScope() as s:
        a, b, c = (s.keep(Fake(n, log)) for n in "abc")
        assert s.release(b) is b
        assert s.release(None) is None              # nothing to take out: an optional buffer that was not made
    assert log == ["c", "a"] and b.freed == 0

    def make():
        with _lib.DeviceScope() as s:
            s.keep(Fake("t", log))
            return s.release(s.keep(Fake("out", log)))
    out = make()
    assert out.freed == 0 and log == ["c", "a", "t"]


def test_a_released_object_stays_when_the_block_fails_later():
    log = []
    with pytest.raises(ValueError):
        with _lib.DeviceScope() as s:
            a, b = s.keep(Fake("a", log)), s.keep(Fake("b", log))
            s.release(a)
            raise ValueError()
    assert log == ["b"] and a.freed == 0


def test_an_object_freed_early_is_not_an_error():
    log = []
    with _lib.DeviceScope() as s:
        a, b = s.keep(Fake("a", log)), s.keep(Fake("b", log))
        a.free()
        assert log == ["a"]
    assert log == ["a", "b"]                        # the scope's own free of `a` is the buffer's no-op


def test_a_free_that_raises_does_not_stop_the_remaining_frees():
    log = []
    with pytest.raises(RuntimeError, match="free of b"):
        with _lib.DeviceScope() as s:
            s.keep(Fake("a", log))
            s.keep(Fake("b", log, fails=True))
            s.keep(Fake("c", log))
    assert log == ["c", "b", "a"]
    # beside an exception of the block, the block's exception is the one that is seen
    log = []
    with pytest.raises(KeyError):
        with _lib.DeviceScope() as s:
            s.keep(Fake("a", log))
            s.keep(Fake("b", log, fails=True))
            raise KeyError("block")
    assert log == ["b", "a"]
