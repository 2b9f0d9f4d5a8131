"""Every HIP stream of the library comes from one factory (cmx_make_stream, cmix_amd/csrc/cmx_api.hip) and goes through
cmx_destroy_stream: only streams made there carry the compute-unit mask that gives each its own hardware queue, and only they are
counted against the device's queue budget (include/cmix_amd.h, CMX_MAX_HW_QUEUES)."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "cmix_amd", "csrc")
CREATE = re.compile(r"\bhip(?:Ext)?StreamCreate\w*\s*\(")
DESTROY = re.compile(r"\bhipStreamDestroy\s*\(")


def _sources():
    for d, _, files in os.walk(CSRC):
        for f in sorted(files):
            if f.endswith((".hip", ".h", ".cpp", ".c", ".hpp")):
                p = os.path.join(d, f)
                with open(p, encoding="utf-8", errors="replace") as fh:
                    yield os.path.relpath(p, CSRC), fh.read()


def _body(text, signature):
    """the text of a function from its signature to the first closing brace at the start of a line"""
    i = text.index(signature)
    return text[i:text.index("\n}\n", i) + 3]


def test_streams_are_created_and_destroyed_only_in_the_factory():
    seen = 0
    for rel, text in _sources():
        if rel == "cmx_api.hip":
            make, destroy = _body(text, "int cmx_make_stream("), _body(text, "void cmx_destroy_stream(")
            assert len(CREATE.findall(make)) == 2 and not DESTROY.findall(make)
            assert len(DESTROY.findall(destroy)) == 1 and not CREATE.findall(destroy)
            text = text.replace(make, "").replace(destroy, "")
            seen += 1
        lines = [(n + 1, l) for n, l in enumerate(text.splitlines()) if CREATE.search(l) or DESTROY.search(l)]
        assert not lines, f"{rel}: HIP streams outside cmx_make_stream / cmx_destroy_stream: {lines}"
    assert seen == 1


def test_factory_streams_carry_a_compute_unit_mask():
    """a plain stream would be pooled onto GPU_MAX_HW_QUEUES shared queues"""
    text = dict(_sources())["cmx_api.hip"]
    make = _body(text, "int cmx_make_stream(")
    assert [m.group(0).split("(")[0] for m in CREATE.finditer(make)] == ["hipExtStreamCreateWithCUMask"] * 2
    assert "CMX_MAX_HW_QUEUES" in make
    assert "setenv(" not in text, "the library does not touch the environment to get its queues"
