"""C ABI: the HIP library loads on a GPU-less host and exports every symbol
include/burgers.h declares (no compute calls here)."""
import ctypes
import os
import re

from conftest import ROOT


def header_symbols():
    text = open(os.path.join(ROOT, "include", "burgers.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(burg_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from finitedifference_amd import _lib
    lib = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(lib, s), f"libburgers_hip.so does not export {s}"
    assert sorted(syms) == sorted(_lib.EXPORTS)


def test_abi_version_and_errors_without_gpu():
    from finitedifference_amd import _lib
    lib = _lib.load()
    assert lib.burg_abi_version() == _lib.ABI_VERSION
    h = ctypes.c_void_p()
    # a null out pointer is rejected before any device call
    assert lib.burg_ctx_create(0, 8, 8, None) == _lib.BURG_EINVAL
    assert b"null" in lib.burg_last_error()
    assert lib.burg_set_options(None, 64, 0, 0.0, 0) == _lib.BURG_EINVAL


def test_built_for_gfx950():
    so = open(os.path.join(ROOT, "finitedifference_amd", "libburgers_hip.so"), "rb").read()
    assert b"gfx950" in so


# the default build's burg_build_flags(): csrc/Makefile's HIPFLAGS (ARCH =
# gfx950) with "| knobs: none" appended (its FLAGSTR)
DEFAULT_FLAGS = ("-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wall "
                 "-Wno-unused-result -Wno-bitwise-instead-of-logical | knobs: none")


def test_flags_are_default_on_literal_strings():
    from finitedifference_amd import _lib
    mk = open(os.path.join(ROOT, "finitedifference_amd", "csrc", "Makefile")).read()
    hipflags = re.search(r"^HIPFLAGS \?= (.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950")
    assert DEFAULT_FLAGS == hipflags.strip() + " | knobs: none"
    assert _lib.flags_are_default(DEFAULT_FLAGS)
    base = DEFAULT_FLAGS[:-len(" | knobs: none")]
    # a variant names its knobs (make VARIANT=cp2 KNOBS="-DBURG_COMM_PRIO=2")
    assert not _lib.flags_are_default(base + " | knobs: -DBURG_COMM_PRIO=2")
    # a knob passed through HIPFLAGS leaves KNOBS empty: still no default build
    assert not _lib.flags_are_default(base + " -DBURG_STORE_WAVE=0 | knobs: none")
    assert not _lib.flags_are_default("-O3 -DBURG_DMA_READBACK=1 --offload-arch=gfx950 | knobs: none")
    # other flags after the knobs field, an empty string, a knob-less variant marker
    assert not _lib.flags_are_default(DEFAULT_FLAGS + " -g")
    assert not _lib.flags_are_default("")
    assert not _lib.flags_are_default(base + " | knobs: -DNDEBUG")
    # a non-BURG define in HIPFLAGS is not a knob
    assert _lib.flags_are_default(base + " -DNDEBUG | knobs: none")
