"""The read path's host-side checks (no GPU): the Python chunk.Reader rejects a DataRef that
reaches past its chunk before any GPU context exists, and the ABI additions (pfscdc_slice,
pfscdc_read_slices, pfscdc_last_read_timings, pfscdc_store_read) are declared, bound and
exported consistently."""
import ctypes as C
import os
import re

import pytest

from pfs_amd import _lib
from pfs_amd import cdc
from pfs_amd import chunk as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pfscdc.h")
READ_API = ["pfscdc_read_slices", "pfscdc_last_read_timings", "pfscdc_store_read"]


@pytest.fixture
def no_ctx(monkeypatch):
    """Any attempt to create a GPU context fails the test."""
    def boom(*a, **k):
        raise AssertionError("a GPU context was created")
    monkeypatch.setattr(cdc.Chunker, "__init__", boom)


def _dr(ref_size, offset, size):
    ref = pc.Ref(size_bytes=ref_size, edge=False, chunk_index=0, id=bytes(32), dek=bytes(32))
    return pc.DataRef(ref=ref, hash=bytes(32), offset_bytes=offset, size_bytes=size)


@pytest.mark.parametrize("offset,size", [(0, 101), (100, 1), (101, 0), (50, 51), (-1, 1), (0, -1)])
def test_reader_rejects_dataref_past_its_chunk_before_any_gpu_call(no_ctx, offset, size):
    st = pc.Storage(device=0, store=pc.ChunkStore())
    r = st.new_reader([_dr(100, 0, 100), _dr(100, offset, size)])
    with pytest.raises(ValueError):
        r.get()

    class FakeTensor:  # rejected before the tensor is looked at
        pass

    with pytest.raises(ValueError):
        r.get_into(FakeTensor())


def test_reader_iterates_datarefs_in_order(no_ctx):
    drs = [_dr(100, i, 1) for i in range(5)]
    seen = []
    pc.Storage(device=0, store=pc.ChunkStore()).new_reader(drs).iterate(seen.append)
    assert seen == drs


def test_reader_needs_a_store(no_ctx):
    with pytest.raises(ValueError):
        pc.Storage(device=0).new_reader([_dr(100, 0, 1)]).get()


def test_read_api_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name in READ_API:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED
        assert getattr(lib, name).argtypes is not None
    assert len(lib.pfscdc_read_slices.argtypes) == 14
    assert len(lib.pfscdc_store_read.argtypes) == 8


def test_slice_record_layout_matches_header():
    text = open(HEADER).read()
    m = re.search(r"typedef struct pfscdc_slice \{(.*?)\} pfscdc_slice;", text, flags=re.S)
    assert m
    fields = re.findall(r"(uint32_t|uint64_t)\s+(\w+);", m.group(1))
    dt = _lib.slice_dtype()
    assert [n for _, n in fields] == list(dt.names)
    assert [dt[n].itemsize for n in dt.names] == [4 if t == "uint32_t" else 8 for t, _ in fields]
    assert dt.itemsize == 24
    assert (_lib.PFSCDC_ECORRUPT, _lib.PFSCDC_ENOTFOUND) == (-7, -8)
    codes = dict(re.findall(r"#define (PFSCDC_E\w+) (-\d+)", text))
    assert int(codes["PFSCDC_ECORRUPT"]) == _lib.PFSCDC_ECORRUPT
    assert int(codes["PFSCDC_ENOTFOUND"]) == _lib.PFSCDC_ENOTFOUND


def test_store_read_rejects_a_null_ctx():
    lib = _lib.load()
    store = pc.ChunkStore()
    store.put(bytes(32), b"x" * 100)
    arr = (_lib.FullDataRef * 1)()
    arr[0] = pc._full(_dr(100, 0, 10))
    nw = C.c_uint64()
    assert lib.pfscdc_store_read(None, store._s, arr, 1, None, 0, 0, C.byref(nw)) == \
        _lib.PFSCDC_EINVAL
