"""Shared helpers of the header ledgers and argument-error tests (tests/test_*_host.py, tests/test_cabi.py): what a header under include/ declares,
against what cfen_vit_dehazing_amd/_lib.py binds and libcfen_hip.so exports.  No GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions(header):
    """{function: number of parameters} of include/<header>"""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
            for m in re.finditer(r"\b(cfen_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def library():
    """cfen_vit_dehazing_amd._lib, with libcfen_hip.so built if it is not there yet"""
    from cfen_vit_dehazing_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def check_header_bound(header, expected, word=None):
    """include/cfen_<name>.h declares exactly `expected` ({function: number of parameters}); _lib.HEADERS binds exactly those with as many
    argtypes, the library exports them and the loaded functions carry the table's types; `word` (default <name>) does not occur in the frozen
    include/cfen_hip.h; csrc/k_<name>.hip is built.  That no other header's table holds one of the names is tests/test_cabi.py's to check."""
    from cfen_vit_dehazing_amd import build
    _lib = library()
    name = header[len("cfen_"):-len(".h")]
    fns = header_functions(header)
    assert fns == expected
    table = _lib.HEADERS[header]
    assert sorted(table) == sorted(fns)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for sym, nargs in fns.items():
        assert hasattr(raw, sym), "libcfen_hip.so does not export %s" % sym
        res, args = table[sym]
        assert len(args) == nargs, sym
        assert getattr(lib, sym).argtypes == args and getattr(lib, sym).restype == res
    assert (word or name) not in open(os.path.join(ROOT, "include", "cfen_hip.h")).read()
    assert "k_%s.hip" % name in build.SOURCES


def check_guard_band_test_calls(test_file, test_name, symbols):
    """the guard-band test `test_name` of tests/<test_file> calls lib.<symbol>( for every symbol: read from the text, since a GPU test module
    cannot be imported without a device"""
    source = open(os.path.join(ROOT, "tests", test_file)).read()
    body = re.search(r"\ndef %s\(.*?(?=\n(?:def |@pytest|# ----))" % test_name, source, flags=re.S)
    assert body, "tests/%s has no %s" % (test_file, test_name)
    assert symbols
    for sym in symbols:
        assert "lib.%s(" % sym in body.group(0), "%s does not call %s" % (test_name, sym)


def refused(lib, fn, what, *args):
    """cfen_<fn>(*args) is refused before any launch, with an error that names `fn` and says `what` (bytes)"""
    assert getattr(lib, "cfen_" + fn)(*args) == -1
    err = lib.cfen_last_error()
    assert fn.encode() in err and what in err, err


def off(ptr, k):
    """the pointer k bytes after ptr"""
    return ctypes.c_void_p(ptr.value + k)
