"""The third companion library libmi355rec_embed_half.so (include/mi355rec_embed_half.h) as a build product, without a
GPU: it builds for gfx950, exports exactly what its header declares, capi.EMBED_HALF_SIGNATURES binds all of it and shares
no name with the other three tables, it links libmi355rec.so through $ORIGIN and neither companion, no kernel reserves
scratch or leaves the budget of two 512-thread workgroups per CU (128 VGPRs, 64 KiB LDS), and every kernel's figures are
the record in tests/golden/embed_half_kernel_budgets.json, whose rows stand in DESIGN.md §5.4.23.  (That the other three
libraries did not move is what the unchanged metadata tests of each show.)"""
import ctypes
import itertools
import json
import re
import subprocess

import pytest

from tests.test_capi_cpu import declared_symbols


@pytest.fixture(scope="module")
def half_lib_path():
    from spotify_recommender_amd import build
    return build.build_embed_half()


def test_exports_are_the_header_and_the_bindings(half_lib_path, golden_dir):
    from spotify_recommender_amd import build, capi
    root = golden_dir.parents[1]
    declared = declared_symbols(root, "mi355rec_embed_half.h")
    assert declared == sorted(f"mi355rec_embed_half_{x}" for x in ("create", "destroy", "last_error", "query", "scores", "info", "enqueue_probe"))
    syms = subprocess.run([str(build.LLVM_BIN / "llvm-readelf"), "--dyn-syms", "-W", str(half_lib_path)], capture_output=True, text=True,
                          check=True).stdout
    # (Num: Value Size Type Bind Vis Ndx Name; Ndx UND = imported from libmi355rec.so, not exported)
    exported = sorted({f[7].split("@")[0] for f in (line.split() for line in syms.splitlines())
                       if len(f) >= 8 and f[6] != "UND" and re.match(r"mi355rec_", f[7])})
    assert exported == declared, "the library exports something its header does not declare, or the reverse"
    assert set(capi.EMBED_HALF_SIGNATURES) == set(declared)
    tables = [capi.SIGNATURES, capi.EMBED_SIGNATURES, capi.EMBED_BATCH_SIGNATURES, capi.EMBED_HALF_SIGNATURES]
    for a, b in itertools.combinations(tables, 2):
        assert not set(a) & set(b), "the four tables are pairwise disjoint"
    L = capi.embed_half_lib()
    for name, (_, argtypes) in capi.EMBED_HALF_SIGNATURES.items():
        assert getattr(L, name).argtypes == argtypes, name
    assert ctypes.sizeof(capi.EmbedHalfInfo) == 64 and capi.EmbedHalfInfo.storage.offset == ctypes.sizeof(capi.EmbedInfo) == 56
    header = (root / "include" / "mi355rec_embed_half.h").read_text()
    for name, value in (("FP16", capi.EMBED_HALF_FP16), ("BF16", capi.EMBED_HALF_BF16)):
        assert f"#define MI355REC_EMBED_HALF_{name} {value}\n" in header


def test_it_links_against_the_product_library_beside_it(half_lib_path):
    from spotify_recommender_amd import build
    dyn = subprocess.run([str(build.LLVM_BIN / "llvm-readelf"), "-d", str(half_lib_path)], capture_output=True, text=True, check=True).stdout
    assert "libmi355rec.so" in dyn and "$ORIGIN" in dyn
    assert "libmi355rec_embed.so" not in dyn and "libmi355rec_embed_batch.so" not in dyn, "the companions share nothing but the product library"


def test_a_null_handle_is_refused(half_lib_path):
    from spotify_recommender_amd import capi
    L = capi.embed_half_lib()
    e = ctypes.c_void_p()
    words = (ctypes.c_uint16 * 16)()
    for storage in (capi.EMBED_HALF_FP16, capi.EMBED_HALF_BF16):
        assert L.mi355rec_embed_half_create(None, words, 1, 16, storage, ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
        assert b"null argument" in L.mi355rec_embed_half_last_error(None)
    assert L.mi355rec_embed_half_create(ctypes.c_void_p(16), words, 1, 16, 0, None) == capi.ERR_INVALID_ARG   # (out is looked at first)
    assert L.mi355rec_embed_half_query(None, None, None) == capi.ERR_INVALID_ARG
    assert L.mi355rec_embed_half_scores(None, None, None, None) == capi.ERR_INVALID_ARG
    assert L.mi355rec_embed_half_info(None, None) == capi.ERR_INVALID_ARG
    assert L.mi355rec_embed_half_enqueue_probe(None, None, None) == capi.ERR_INVALID_ARG
    L.mi355rec_embed_half_destroy(None)


def test_kernels_are_gfx950_scratch_free_and_on_budget(half_lib_path, golden_dir):
    from spotify_recommender_amd import build
    golden = json.loads((golden_dir / "embed_half_kernel_budgets.json").read_text())
    assert build.check_no_scratch(half_lib_path) == len(golden)
    meta = {k["name"]: k for k in build.kernel_metadata(half_lib_path)}
    assert sorted(meta) == sorted(g["name"] for g in golden), "a kernel came or went"
    scans = sorted(g["label"] for g in golden if g["label"].startswith("embed_half_scan_kernel<"))
    assert scans == sorted(f"embed_half_scan_kernel<{d}, {s}>" for d in (16, 32, 64, 128) for s in ("fp16", "bf16")), scans
    design = (golden_dir.parents[1] / "DESIGN.md").read_text()
    section = design[design.index("### 5.4.23"):]
    section = section[: section.index("\n## ")] if "\n## " in section else section
    for g in golden:
        k = meta[g["name"]]
        assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] <= 65536, (g["label"], k)
        assert (k["vgpr"], k["lds"]) == (g["vgpr"], g["lds"]), (g["label"], k)
        row = f"| `{g['label']}` | {g['vgpr']} | {g['lds']} |"
        assert row in section, f"DESIGN.md §5.4.23 does not carry the row {row}"
