"""The in-reference-tree branch of the headers INTEGRATION.md §2 hands a
maintainer (PSKV_IN_REFERENCE_TREE), compiled against the reference's own
boundary types where the image allows it.

  include/ps/host_frames.hpp  built by the package build (oracle/Makefile's
                              in-tree target, into oracle/_ref/) against
                              base/third_party/sarray.h and base/message.hpp
                              (neither needs glog) and linked against
                              libpskv.so: tests/cpp/in_tree_frames.cpp
  include/ps/hip_storage.hpp  NOT built: its in-tree branch includes
                              server/abstract_storage.hpp, which includes
                              glog/logging.h, absent from the image (and a
                              stand-in header is not allowed); INTEGRATION.md §2
                              records it

CPU only (compile + link; running needs a GPU for pskv_host_alloc).  The test
reads what the build left in oracle/_ref/; it skips where the build had no
reference tree to compile against."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OUT = os.path.join(ROOT, "oracle", "_ref")


def test_host_frames_in_reference_tree():
    lib = os.path.join(ROOT, "parameter_server_amd", "libpskv.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build())"
    out, deps_file = os.path.join(REF_OUT, "in_tree_frames"), os.path.join(REF_OUT, "in_tree_frames.d")
    if not os.path.exists(deps_file):
        pytest.skip("reference tree absent when the package was built")
    assert os.path.exists(out) and os.access(out, os.X_OK)
    # the reference's own header, not the restatement, was compiled
    with open(deps_file) as f:
        deps = f.read()
    assert "base/third_party/sarray.h" in deps and "ps/sarray.hpp" not in deps
    assert "include/ps/host_frames.hpp" in deps


def test_hip_storage_in_tree_branch_is_recorded():
    # the branch that cannot be built here is named in INTEGRATION.md
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert "glog/logging.h" in text and "in_tree_frames.cpp" in text
