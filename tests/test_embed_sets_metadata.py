"""The fourth companion library libmi355rec_embed_sets.so (include/mi355rec_embed_sets.h) as a build product, without a
GPU: it builds for gfx950, exports exactly what its header declares, capi.EMBED_SETS_SIGNATURES binds all of it and shares
no name with the other four tables, it links libmi355rec.so through $ORIGIN and no other companion, NULL arguments are
refused, no kernel reserves scratch or leaves the budget of two 512-thread workgroups per CU (128 VGPRs, 64 KiB LDS), and
every kernel's figures are the record in tests/golden/embed_sets_kernel_budgets.json, whose rows stand in DESIGN.md
§5.4.26.  (That the other three libraries did not move under the scan body's restriction policy is what the unchanged
metadata tests of each show.)"""
import ctypes
import itertools
import json
import re
import subprocess

import pytest

from tests.test_capi_cpu import declared_symbols

ENTRY_POINTS = ("create", "create_half", "destroy", "last_error", "info", "rowset_create", "rowset_create_mask", "rowset_add",
                "rowset_count", "rowset_destroy", "query")


@pytest.fixture(scope="module")
def sets_lib_path():
    from spotify_recommender_amd import build
    return build.build_embed_sets()


def test_exports_are_the_header_and_the_bindings(sets_lib_path, golden_dir):
    from spotify_recommender_amd import build, capi
    root = golden_dir.parents[1]
    declared = declared_symbols(root, "mi355rec_embed_sets.h")
    assert declared == sorted(f"mi355rec_embed_sets_{x}" for x in ENTRY_POINTS)
    syms = subprocess.run([str(build.LLVM_BIN / "llvm-readelf"), "--dyn-syms", "-W", str(sets_lib_path)], capture_output=True, text=True,
                          check=True).stdout
    # (Num: Value Size Type Bind Vis Ndx Name; Ndx UND = imported from libmi355rec.so, not exported)
    exported = sorted({f[7].split("@")[0] for f in (line.split() for line in syms.splitlines())
                       if len(f) >= 8 and f[6] != "UND" and re.match(r"mi355rec_", f[7])})
    assert exported == declared, "the library exports something its header does not declare, or the reverse"
    assert set(capi.EMBED_SETS_SIGNATURES) == set(declared)
    tables = [capi.SIGNATURES, capi.EMBED_SIGNATURES, capi.EMBED_BATCH_SIGNATURES, capi.EMBED_HALF_SIGNATURES, capi.EMBED_SETS_SIGNATURES]
    for a, b in itertools.combinations(tables, 2):
        assert not set(a) & set(b), "the five tables are pairwise disjoint"
    L = capi.embed_sets_lib()
    for name, (_, argtypes) in capi.EMBED_SETS_SIGNATURES.items():
        assert getattr(L, name).argtypes == argtypes, name
    assert ctypes.sizeof(capi.EmbedSetsExt) == 24 and capi.EmbedSetsExt.only.offset == 16
    assert ctypes.sizeof(capi.EmbedSetsInfo) == 88 and capi.EmbedSetsInfo.tiles_total.offset == ctypes.sizeof(capi.EmbedHalfInfo) == 64
    assert capi.EMBED_SETS_FP32 == -1


def test_it_links_against_the_product_library_beside_it(sets_lib_path):
    from spotify_recommender_amd import build
    dyn = subprocess.run([str(build.LLVM_BIN / "llvm-readelf"), "-d", str(sets_lib_path)], capture_output=True, text=True, check=True).stdout
    assert "libmi355rec.so" in dyn and "$ORIGIN" in dyn
    for other in ("libmi355rec_embed.so", "libmi355rec_embed_batch.so", "libmi355rec_embed_half.so"):
        assert other not in dyn, "the companions share nothing but the product library"


def test_null_arguments_are_refused(sets_lib_path):
    from spotify_recommender_amd import capi
    L = capi.embed_sets_lib()
    e, s = ctypes.c_void_p(), ctypes.c_void_p()
    table = (ctypes.c_float * 16)()
    words = (ctypes.c_uint16 * 16)()
    assert L.mi355rec_embed_sets_create(None, table, 1, 16, ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
    assert b"null argument" in L.mi355rec_embed_sets_last_error(None)
    for storage in (capi.EMBED_HALF_FP16, capi.EMBED_HALF_BF16):
        assert L.mi355rec_embed_sets_create_half(None, words, 1, 16, storage, ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
    assert L.mi355rec_embed_sets_create(ctypes.c_void_p(16), table, 1, 16, None) == capi.ERR_INVALID_ARG   # (out is looked at first)
    assert L.mi355rec_embed_sets_create_half(ctypes.c_void_p(16), words, 1, 16, 0, None) == capi.ERR_INVALID_ARG
    assert L.mi355rec_embed_sets_create_half(ctypes.c_void_p(16), words, 1, 16, -1, ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
    assert b"storage -1" in L.mi355rec_embed_sets_last_error(None)   # (fp32 is mi355rec_embed_sets_create's)
    assert L.mi355rec_embed_sets_query(None, None, None, None) == capi.ERR_INVALID_ARG
    assert L.mi355rec_embed_sets_info(None, None) == capi.ERR_INVALID_ARG
    ids = (ctypes.c_int64 * 1)(0)
    assert L.mi355rec_embed_sets_rowset_create(None, ids, 1, ctypes.byref(s)) == capi.ERR_INVALID_ARG and not s
    assert L.mi355rec_embed_sets_rowset_create_mask(None, None, 0, ctypes.byref(s)) == capi.ERR_INVALID_ARG and not s
    assert L.mi355rec_embed_sets_rowset_add(None, ids, 1) == capi.ERR_INVALID_ARG
    assert L.mi355rec_embed_sets_rowset_count(None) == -1
    L.mi355rec_embed_sets_rowset_destroy(None)
    L.mi355rec_embed_sets_destroy(None)


def test_kernels_are_gfx950_scratch_free_and_on_budget(sets_lib_path, golden_dir):
    from spotify_recommender_amd import build
    golden = json.loads((golden_dir / "embed_sets_kernel_budgets.json").read_text())
    assert build.check_no_scratch(sets_lib_path) == len(golden)
    meta = {k["name"]: k for k in build.kernel_metadata(sets_lib_path)}
    assert sorted(meta) == sorted(g["name"] for g in golden), "a kernel came or went"
    scans = sorted(g["label"] for g in golden if g["label"].startswith("embed_sets_scan_kernel<"))
    assert scans == sorted(f"embed_sets_scan_kernel<{s}, {d}>" for d in (16, 32, 64, 128) for s in ("f32", "fp16", "bf16")), scans
    design = (golden_dir.parents[1] / "DESIGN.md").read_text()
    section = design[design.index("### 5.4.26"):]
    section = section[: section.index("\n## ")] if "\n## " in section else section
    for g in golden:
        k = meta[g["name"]]
        assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] <= 65536, (g["label"], k)
        assert (k["vgpr"], k["lds"]) == (g["vgpr"], g["lds"]), (g["label"], k)
        row = f"| `{g['label']}` | {g['vgpr']} | {g['lds']} |"
        assert row in section, f"DESIGN.md §5.4.26 does not carry the row {row}"
