"""amdmsm_multi_exp_batch_items / amdmsm_msm_device_batch_items without a device: the symbols exist, the ABI version
did not move, and the Python mirror of amdmsm_batch_item has the layout the C header gives it."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "amdmsm.h")
NEW_SYMBOLS = ["amdmsm_multi_exp_batch_items", "amdmsm_msm_device_batch_items"]


@pytest.fixture(scope="module")
def lib():
    import libff_amd
    from libff_amd import build

    if not os.path.exists(libff_amd.engine.SO_PATH):
        build.build()
    return ctypes.CDLL(libff_amd.engine.SO_PATH)


@pytest.mark.parametrize("symbol", NEW_SYMBOLS)
def test_symbol_is_exported_and_declared(lib, symbol):
    assert hasattr(lib, symbol), f"{symbol} is not exported by libamdmsm.so"
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % symbol, text), f"{symbol} is not declared in amdmsm.h"
    import libff_amd.engine as e

    assert symbol in e.EXPORTED_SYMBOLS


def test_abi_version_is_still_3(lib):
    import libff_amd.engine as e

    assert lib.amdmsm_abi_version() == 3 and e.ABI_VERSION == 3
    assert re.search(r"#define\s+AMDMSM_ABI_VERSION\s+3\b", open(HEADER).read())


def test_batch_item_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of amdmsm_batch_item, as a C probe compiled against the header prints them."""
    import libff_amd.engine as e

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    fields = [f[0] for f in e.BatchItemStruct._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "amdmsm.h"\nint main(void) {\n'
                   '    amdmsm_batch_item it = AMDMSM_BATCH_ITEM_INIT;\n'
                   '    printf("%zu %u", sizeof(amdmsm_batch_item), it.struct_size);\n' +
                   "".join('    printf(" %%zu", offsetof(amdmsm_batch_item, %s));\n' % f for f in fields) +
                   '    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == got[1] == ctypes.sizeof(e.BatchItemStruct)
    assert got[2:] == [getattr(e.BatchItemStruct, f).offset for f in fields]


def test_public_names():
    import libff_amd

    assert hasattr(libff_amd, "BatchItem")
    assert hasattr(libff_amd.Engine, "multi_exp_batch_items") and hasattr(libff_amd.Engine, "msm_device_batch_items")
