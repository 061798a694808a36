"""CPU, no build: every quoted #include of the library's translation units and shared headers is a file the build
hashes (`_lib._source_hash`), so that no header edit leaves stale objects behind an unchanged `.srchash`."""
import os
import re

from gadfly_amd import _lib

INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)


def quoted_includes(path):
    with open(path) as fh:
        return [os.path.normpath(os.path.join(os.path.dirname(path), name)) for name in INCLUDE.findall(fh.read())]


def test_every_quoted_include_is_hashed_by_the_build():
    hashed = {os.path.normpath(p) for p in [_lib.HEADER] + _lib._DEPS}
    seen = 0
    for path in _lib.SOURCES + _lib._DEPS:
        assert os.path.isfile(path), path
        for inc in quoted_includes(path):
            seen += 1
            assert inc in hashed, f"{os.path.basename(path)} includes {inc}, which is not in _lib._DEPS"
    assert seen >= 2 * len(_lib.SOURCES)         # (the parse found them: each unit has the C header and gf_internal.h)


def test_every_hashed_header_is_included_by_something():
    used = {inc for path in _lib.SOURCES + _lib._DEPS for inc in quoted_includes(path)}
    for dep in _lib._DEPS:
        assert os.path.normpath(dep) in used, f"{dep} is hashed into every object but included nowhere"
