"""The second companion library libmi355rec_embed_batch.so (include/mi355rec_embed_batch.h) as a build product, without a
GPU: it builds for gfx950, exports exactly what its header declares, capi.EMBED_BATCH_SIGNATURES binds all of it and shares
no name with the other two tables, it links libmi355rec.so through $ORIGIN, no kernel reserves scratch or leaves the
budget of two 512-thread workgroups per CU (128 VGPRs, 64 KiB LDS), and every kernel's figures are the record in
tests/golden/embed_batch_kernel_budgets.json, whose rows stand in DESIGN.md §5.4.22.  (That the other two libraries did
not move is what the unchanged tests/test_embed_metadata.py and tests/test_kernel_metadata.py show.)"""
import ctypes
import json
import re
import subprocess

import pytest

from tests.test_capi_cpu import declared_symbols


@pytest.fixture(scope="module")
def batch_lib_path():
    from spotify_recommender_amd import build
    return build.build_embed_batch()


def test_exports_are_the_header_and_the_bindings(batch_lib_path, golden_dir):
    from spotify_recommender_amd import build, capi
    root = golden_dir.parents[1]
    declared = declared_symbols(root, "mi355rec_embed_batch.h")
    assert declared == sorted(f"mi355rec_embed_batch_{x}" for x in ("create", "destroy", "last_error", "query", "info"))
    syms = subprocess.run([str(build.LLVM_BIN / "llvm-readelf"), "--dyn-syms", "-W", str(batch_lib_path)], capture_output=True, text=True,
                          check=True).stdout
    # (Num: Value Size Type Bind Vis Ndx Name; Ndx UND = imported from libmi355rec.so, not exported)
    exported = sorted({f[7].split("@")[0] for f in (line.split() for line in syms.splitlines())
                       if len(f) >= 8 and f[6] != "UND" and re.match(r"mi355rec_", f[7])})
    assert exported == declared, "the library exports something its header does not declare, or the reverse"
    assert set(capi.EMBED_BATCH_SIGNATURES) == set(declared)
    assert not set(capi.EMBED_BATCH_SIGNATURES) & (set(capi.SIGNATURES) | set(capi.EMBED_SIGNATURES)), "the third table is disjoint from the other two"
    L = capi.embed_batch_lib()
    for name, (_, argtypes) in capi.EMBED_BATCH_SIGNATURES.items():
        assert getattr(L, name).argtypes == argtypes, name
    assert ctypes.sizeof(capi.EmbedBatchQuery) == 48 and ctypes.sizeof(capi.EmbedBatchResult) == 32 and ctypes.sizeof(capi.EmbedBatchInfo) == 56
    assert capi.EmbedBatchQuery.n_users.offset == 32 and capi.EmbedBatchQuery.w_embed.offset == 44
    assert capi.EmbedBatchInfo.pass_users.offset == 36
    header = (root / "include" / "mi355rec_embed_batch.h").read_text()
    for name, value in (("MAX_USERS", capi.EMBED_BATCH_MAX_USERS), ("MAX_TOPN", capi.EMBED_BATCH_MAX_TOPN), ("MAX_EXCLUDE", capi.EMBED_BATCH_MAX_EXCLUDE)):
        assert f"#define MI355REC_EMBED_BATCH_{name} {value}\n" in header


def test_it_links_against_the_product_library_beside_it(batch_lib_path):
    from spotify_recommender_amd import build
    dyn = subprocess.run([str(build.LLVM_BIN / "llvm-readelf"), "-d", str(batch_lib_path)], capture_output=True, text=True, check=True).stdout
    assert "libmi355rec.so" in dyn and "$ORIGIN" in dyn
    assert "libmi355rec_embed.so" not in dyn, "the two companions share nothing but the product library"


def test_a_null_handle_is_refused(batch_lib_path):
    from spotify_recommender_amd import capi
    L = capi.embed_batch_lib()
    e = ctypes.c_void_p()
    table = (ctypes.c_float * 16)()
    assert L.mi355rec_embed_batch_create(None, table, 1, 16, ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
    assert b"null argument" in L.mi355rec_embed_batch_last_error(None)
    assert L.mi355rec_embed_batch_query(None, None, None) == capi.ERR_INVALID_ARG
    assert L.mi355rec_embed_batch_info(None, None) == capi.ERR_INVALID_ARG
    L.mi355rec_embed_batch_destroy(None)


def test_kernels_are_gfx950_scratch_free_and_on_budget(batch_lib_path, golden_dir):
    from spotify_recommender_amd import build
    golden = json.loads((golden_dir / "embed_batch_kernel_budgets.json").read_text())
    assert build.check_no_scratch(batch_lib_path) == len(golden)
    meta = {k["name"]: k for k in build.kernel_metadata(batch_lib_path)}
    assert sorted(meta) == sorted(g["name"] for g in golden), "a kernel came or went"
    scans = [g["label"] for g in golden if g["label"].startswith("embed_batch_scan_kernel<")]
    assert sorted(s.split("<")[1].split(",")[0] for s in scans) == sorted(["16", "32", "64", "128"], key=str), scans
    design = (golden_dir.parents[1] / "DESIGN.md").read_text()
    section = design[design.index("### 5.4.22"):]
    section = section[: section.index("\n## ")] if "\n## " in section else section
    for g in golden:
        k = meta[g["name"]]
        assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] <= 65536, (g["label"], k)
        assert (k["vgpr"], k["lds"]) == (g["vgpr"], g["lds"]), (g["label"], k)
        row = f"| `{g['label']}` | {g['vgpr']} | {g['lds']} |"
        assert row in section, f"DESIGN.md §5.4.22 does not carry the row {row}"
