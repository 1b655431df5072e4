"""csrc/Makefile holds the ONE list of the library's sources: SRCS is what gets compiled and linked, SRCS + HDRS is what the
build-provenance hash covers (fanlin_rs_amd.source_hash, flgpu_build_info) and what every object depends on.  A file in csrc/ that
is missing from the lists is either not linked or -- a header -- escapes the hash that exists to say "this library was built
from these sources".  No GPU and no library needed."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fanlin-rs_amd", "csrc")
GENERATED = {"fl_buildinfo.gen.cpp"}  # written by the Makefile's fl_buildinfo.o rule


def _make_list(name):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^%s\s*=\s*(.*)$" % name, mk, re.M).group(1).split()


def _on_disk(*suffixes):
    return {f for f in os.listdir(CSRC) if f.endswith(suffixes)} - GENERATED


def test_every_source_file_is_in_srcs():
    srcs = _make_list("SRCS")
    assert len(srcs) == len(set(srcs)), "SRCS names a file twice"
    assert _on_disk(".hip", ".cpp") == set(srcs)


def test_every_header_is_in_hdrs():
    hdrs = _make_list("HDRS")
    assert len(hdrs) == len(set(hdrs)), "HDRS names a file twice"
    assert _on_disk(".h") == {h for h in hdrs if "/" not in h}, "a header of csrc/ is not hashed (or HDRS names one that is gone)"


def test_every_listed_file_exists():
    missing = [f for f in _make_list("SRCS") + _make_list("HDRS") if not os.path.isfile(os.path.join(CSRC, f))]
    assert not missing, missing
