"""tg_ns_out grew a field (rows_prefilled, appended): the C header and the ctypes mirror must agree on the struct's size
and on where the field lies, or every launch reads a pitch for a flag.  A C program compiled against include/tchgeo.h
prints both numbers.  tg_ns_rows_fill refuses null and negative arguments on the host, before any launch, so that is
checked here too (no GPU is touched)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TG_ERR_INVALID = 1

PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "tchgeo.h"
int main(void) {
    tg_ns_out o = {0};
    printf("%zu %zu %zu %lld\n", sizeof(tg_ns_out), offsetof(tg_ns_out, rows_prefilled), offsetof(tg_ns_out, cap_edges),
           (long long)o.rows_prefilled);
    return 0;
}
"""


@pytest.fixture(scope="module")
def cabi():
    if not os.path.exists(os.path.join(ROOT, "tch-geometric_amd", "lib", "libtchgeo_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tch-geometric_amd"), "-s"])
    from tch_geometric import _cabi
    return _cabi


def test_header_and_ctypes_agree_on_tg_ns_out(cabi, tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc, "a C compiler is needed (the oracle is built with one)"
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(PROGRAM)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_flag, off_cap, zero = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert zero == 0
    assert size == C.sizeof(cabi.TgNsOut)
    assert off_flag == cabi.TgNsOut.rows_prefilled.offset
    assert off_cap == cabi.TgNsOut.cap_edges.offset
    assert off_flag == off_cap + 8 and size == off_flag + 8          # appended: nothing before it moved
    assert cabi.TgNsOut().rows_prefilled == 0                        # a struct built without the field says "off"


def test_rows_fill_refuses_bad_arguments_before_any_launch(cabi):
    fill = cabi.lib.tg_ns_rows_fill
    ok_ptr = C.c_void_p(0x100000)                                    # never dereferenced: every call below is refused
    i64 = C.c_int64
    assert fill(C.c_void_p(0), i64(4), i64(16), i64(8), C.c_void_p(0)) == TG_ERR_INVALID
    assert b"tg_ns_rows_fill" in cabi.lib.tg_last_error()
    assert fill(ok_ptr, i64(-1), i64(16), i64(8), C.c_void_p(0)) == TG_ERR_INVALID
    assert fill(ok_ptr, i64(4), i64(-16), i64(8), C.c_void_p(0)) == TG_ERR_INVALID
    assert fill(ok_ptr, i64(4), i64(16), i64(-8), C.c_void_p(0)) == TG_ERR_INVALID
    assert fill(C.c_void_p(0x100004), i64(4), i64(16), i64(8), C.c_void_p(0)) == TG_ERR_INVALID     # not 8-byte aligned
    assert fill(ok_ptr, i64(1 << 40), i64(1 << 40), i64(8), C.c_void_p(0)) == TG_ERR_INVALID        # size overflows int64
    with pytest.raises(cabi.TchGeoError):
        cabi.check(fill(C.c_void_p(0), i64(4), i64(16), i64(8), C.c_void_p(0)))
    assert "tg_ns_rows_fill" in cabi.EXPORTS


def test_struct_of_an_object_with_the_old_attributes_only(cabi):
    """NsBatchedOut.struct on an object that only mimics NsBatchedOut (no n_seeds, plain attributes): the field stays 0."""
    class T:
        def __init__(self, p):
            self.p, self.shape = p, (3, 7)

        def data_ptr(self):
            return self.p

    class Old:
        samples, rows, cols, edge_index = T(0x1000), T(0x2000), T(0x3000), T(0x4000)
        layer_offsets, counts, states = T(0x5000), T(0x6000), None

    s = cabi.NsBatchedOut.struct(Old())
    assert s.rows_prefilled == 0 and s.rows == 0x2000 and s.cap_edges == 7
    Old.n_seeds = 5
    assert cabi.NsBatchedOut.struct(Old()).rows_prefilled == 0      # n_seeds but no mark on the slab
