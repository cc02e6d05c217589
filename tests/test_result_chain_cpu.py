"""The three helpers every family behind a render build goes through in harry_amd/codec.py -- the chain of builds, the reader of a
handle's named buffers, the stat of a handle -- against a stand-in for the native library that records its calls.  No GPU: the
helpers take the library as an argument."""
import types

import pytest

from harry_amd import codec as hc


class StubLib:
    """hry_<family>_build / _free / _get / _stat / _summary of any family: handles are numbered from 1 in the order they are built"""

    def __init__(self, fail_build=(), widths=None):
        self.calls, self.built, self.fail_build = [], 0, set(fail_build)
        self.widths = widths or {}   # name -> width of the buffers the handles have (others: 1)

    def __getattr__(self, entry):
        family, what = entry[len("hry_"):].rsplit("_", 1)
        if entry == "hry_render_build_ex":
            family, what = "render", "build"
        return lambda *args: getattr(self, "_" + what)(family, *args)

    def _build(self, family, codec_h, mesh_h, *args):
        if family in self.fail_build:
            self.calls.append(("build fails", family))
            raise RuntimeError(f"no {family}")
        self.built += 1
        args[-1]._obj.value = self.built
        self.calls.append(("build", family, self.built, tuple(a.value if hasattr(a, "value") else a for a in args[:-1])))
        return 0

    def _free(self, family, h):
        self.calls.append(("free", family, h.value))

    def _get(self, family, h, name, dev, rows, width, typ):
        self.calls.append(("get", family, name.decode()))
        rows._obj.value, width._obj.value, typ._obj.value = 5, self.widths.get(name.decode(), 1), 4
        return 0

    def _stat(self, family, h, device_ms, uploaded):
        device_ms._obj.value, uploaded._obj.value = 1.5, 7
        return 0

    def _summary(self, family, h, words):
        self.calls.append(("summary", family, len(words)))
        for i in range(len(words)):
            words[i] = 10 + i
        return 0

    def freed(self):
        return [c[1:] for c in self.calls if c[0] == "free"]


def chain(lib):
    return hc._Chain(types.SimpleNamespace(h=101), types.SimpleNamespace(h=202), lib)


def test_a_failing_build_frees_what_was_built_in_reverse():
    lib = StubLib(fail_build={"shells"})
    with pytest.raises(RuntimeError, match="no shells"):
        with chain(lib) as ch:
            r = ch.build("render")
            e = ch.build("edges", r, 3)
            ch.build("shells", r, e, 0)
    assert lib.calls == [("build", "render", 1, ()), ("build", "edges", 2, (1, 3)), ("build fails", "shells"), ("free", "edges", 2), ("free", "render", 1)]


def test_every_handle_is_available_and_freed_once_in_reverse():
    lib = StubLib()
    with chain(lib) as ch:
        r = ch.build("render", 6, entry="hry_render_build_ex")
        e = ch.build("edges", r, 0)
        c = ch.build("creases", r, e, 0.5, 1)
        assert [h.value for h in (r, e, c)] == [1, 2, 3] and [f for f, _ in ch.held] == ["render", "edges", "creases"]
        assert lib.freed() == []
    assert lib.calls[:3] == [("build", "render", 1, (6,)), ("build", "edges", 2, (1, 0)), ("build", "creases", 3, (1, 2, 0.5, 1))]
    assert lib.freed() == [("creases", 3), ("edges", 2), ("render", 1)]
    ch.free()
    assert len(lib.freed()) == 3   # (nothing is freed twice)


def test_a_failing_fill_frees_every_handle_the_familys_own_last():
    """as Codec._topology reads: the inputs go before the buffers are read, the family's own handle when the reading is over"""
    lib = StubLib()

    def fill(family, name, rows, width, typ, h):
        raise ValueError("no room")
    with pytest.raises(ValueError, match="no room"):
        with chain(lib) as ch:
            r = ch.build("render")
            e = ch.build("edges", r, 0)
            o = ch.build("orient", r, e, 2)
            ch.free(keep_last=True)
            assert lib.freed() == [("edges", 2), ("render", 1)]
            hc._read_buffers(lib, "orient", o, ("tri_patch",), fill)
    assert lib.freed() == [("edges", 2), ("render", 1), ("orient", 3)]
    # ... and as the tangents and creases read, with the inputs still held: the reverse of the builds
    lib = StubLib()
    with pytest.raises(ValueError, match="no room"):
        with chain(lib) as ch:
            t = ch.build("tangents", ch.build("render"), 0)
            hc._read_buffers(lib, "tangents", t, ("tangents",), fill)
    assert lib.freed() == [("tangents", 2), ("render", 1)]


def test_take_leaves_the_last_handle_to_the_caller():
    lib = StubLib()
    with chain(lib) as ch:
        ch.build("bvh", ch.build("render"), 0)
        b = ch.take()
    assert b.value == 2 and lib.freed() == [("render", 1)]


def test_the_reader_keeps_the_order_and_skips_what_is_not_there():
    lib = StubLib(widths={"edge_length": 0, "edges": 2})
    seen = []

    def fill(family, name, rows, width, typ, h):
        seen.append((family, name, rows, width, typ, h))
        return name.upper()
    out = hc._read_buffers(lib, "edges", 9, ("tri_edges", "edge_length", "edges", "edge_sides"), fill)
    assert list(out.items()) == [("tri_edges", "TRI_EDGES"), ("edges", "EDGES"), ("edge_sides", "EDGE_SIDES")]
    assert seen == [("edges", "tri_edges", 5, 1, 4, 9), ("edges", "edges", 5, 2, 4, 9), ("edges", "edge_sides", 5, 1, 4, 9)]
    assert [c[2] for c in lib.calls if c[0] == "get"] == ["tri_edges", "edge_length", "edges", "edge_sides"]


@pytest.mark.parametrize("family,words", [("edges", 4), ("shells", 6), ("bvh", 6)])
def test_the_stat_maps_the_summary_words_to_the_keys_in_order(family, words):
    lib = StubLib()
    keys = ("first", "second", "third", "fourth")
    out = hc._read_stat(lib, family, 9, keys, {"extra": 0.25})
    assert list(out.items()) == [("device_ms", 1.5), ("uploaded_bytes", 7), ("extra", 0.25), ("first", 10), ("second", 11), ("third", 12), ("fourth", 13)]
    assert all(type(out[k]) is int for k in keys + ("uploaded_bytes",)) and type(out["device_ms"]) is float
    assert [c for c in lib.calls if c[0] == "summary"] == [("summary", family, words)]
    # a family without a summary (render): the two figures alone, no summary asked for
    lib = StubLib()
    assert hc._read_stat(lib, "render", 9) == {"device_ms": 1.5, "uploaded_bytes": 7} and lib.calls == []
