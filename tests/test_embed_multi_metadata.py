"""The seventh companion library libmi355rec_embed_multi.so (include/mi355rec_embed_multi.h) as a build product, without a
GPU: it builds for gfx950, exports exactly what its header declares, capi.EMBED_MULTI_SIGNATURES binds all of it and shares
no name with the other seven tables, it links libmi355rec.so through $ORIGIN and no other companion, NULL arguments are
refused, its kernels are the twelve scans, the finish and what the shared headers instantiate, no kernel reserves scratch or
leaves the budget of two 512-thread workgroups per CU (128 VGPRs, 64 KiB LDS), every kernel's figures are the record in
tests/golden/embed_multi_kernel_budgets.json, whose rows stand in DESIGN.md §5.4.30, and the kernels it shares with the
stream library come out at that library's recorded figures."""
import ctypes
import itertools
import json
import re
import subprocess

import pytest

from tests.test_capi_cpu import declared_symbols

ENTRY_POINTS = ("create", "create_device", "destroy", "last_error", "info", "enqueue_query")
SHARED = ("merge_kernel", "embed_stream_prepare_kernel", "embed_stream_finish_kernel", "embed_user_kernel", "embed_probe_kernel",
          "embed_half_user_kernel")


@pytest.fixture(scope="module")
def multi_lib_path():
    from spotify_recommender_amd import build
    return build.build_embed_multi()


def test_exports_are_the_header_and_the_bindings(multi_lib_path, golden_dir):
    from spotify_recommender_amd import build, capi
    root = golden_dir.parents[1]
    declared = declared_symbols(root, "mi355rec_embed_multi.h")
    assert declared == sorted(f"mi355rec_embed_multi_{x}" for x in ENTRY_POINTS)
    syms = subprocess.run([str(build.LLVM_BIN / "llvm-readelf"), "--dyn-syms", "-W", str(multi_lib_path)], capture_output=True, text=True,
                          check=True).stdout
    # (Num: Value Size Type Bind Vis Ndx Name; Ndx UND = imported from libmi355rec.so, not exported)
    exported = sorted({f[7].split("@")[0] for f in (line.split() for line in syms.splitlines())
                       if len(f) >= 8 and f[6] != "UND" and re.match(r"mi355rec_", f[7])})
    assert exported == declared, "the library exports something its header does not declare, or the reverse"
    imported = sorted({f[7].split("@")[0] for f in (line.split() for line in syms.splitlines())
                       if len(f) >= 8 and f[6] == "UND" and re.match(r"mi355rec_", f[7])})
    assert imported == ["mi355rec_enqueue_scores", "mi355rec_last_error", "mi355rec_stats"], "what the stream library asks of the product library"
    assert set(capi.EMBED_MULTI_SIGNATURES) == set(declared)
    tables = [capi.SIGNATURES, capi.EMBED_SIGNATURES, capi.EMBED_BATCH_SIGNATURES, capi.EMBED_HALF_SIGNATURES, capi.EMBED_SETS_SIGNATURES,
              capi.EMBED_STREAM_SIGNATURES, capi.EMBED_CAND_SIGNATURES, capi.EMBED_MULTI_SIGNATURES]
    for a, b in itertools.combinations(tables, 2):
        assert not set(a) & set(b), "the eight tables are pairwise disjoint"
    L = capi.embed_multi_lib()
    for name, (_, argtypes) in capi.EMBED_MULTI_SIGNATURES.items():
        assert getattr(L, name).argtypes == argtypes, name


def test_struct_sizes_and_offsets():
    from spotify_recommender_amd import capi
    Q, R, I = capi.EmbedMultiQuery, capi.EmbedMultiResult, capi.EmbedMultiInfo
    assert ctypes.sizeof(Q) == 72
    assert [f for f, _ in Q._fields_] == ["size", "flags", "interests_dev", "audio", "exclude_dev", "audio_row", "n_interests", "n_exclude", "topn",
                                          "metric", "w_audio", "w_embed", "reserved"]
    assert [getattr(Q, f).offset for f, _ in Q._fields_] == [0, 4, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60, 64]
    assert ctypes.sizeof(R) == 40 and [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 16, 24, 32]
    assert R._fields_[: len(capi.EmbedStreamResult._fields_)] == capi.EmbedStreamResult._fields_, "the stream result plus one field"
    assert ctypes.sizeof(I) == 96
    assert [getattr(I, f).offset for f, _ in I._fields_] == [0, 4, 8, 16, 24, 28, 32, 36, 40, 48, 56, 64, 72, 76, 80, 84, 88, 92]
    assert I._fields_[: len(capi.EmbedStreamInfo._fields_)] == capi.EmbedStreamInfo._fields_, "info reports what the stream library's reports"
    assert [f for f, _ in I._fields_[len(capi.EmbedStreamInfo._fields_):]] == ["max_interests", "pass_interests", "query_launches", "reserved"]
    assert (capi.EMBED_MULTI_MAX_INTERESTS, capi.EMBED_MULTI_MAX_EXCLUDE) == (32, 1024)
    header = (capi.PKG.parent / "include" / "mi355rec_embed_multi.h").read_text()
    assert "#define MI355REC_EMBED_MULTI_MAX_INTERESTS 32" in header and "#define MI355REC_EMBED_MULTI_MAX_EXCLUDE 1024" in header
    # both identities stand in the header
    assert "1. K = 1." in header and "bit for bit, what mi355rec_embed_stream_enqueue_query leaves" in header
    assert "2. Any K." in header and "prefer the lower k at equal" in header


def test_it_links_against_the_product_library_beside_it(multi_lib_path):
    from spotify_recommender_amd import build
    dyn = subprocess.run([str(build.LLVM_BIN / "llvm-readelf"), "-d", str(multi_lib_path)], capture_output=True, text=True, check=True).stdout
    assert "libmi355rec.so" in dyn and "$ORIGIN" in dyn
    for other in ("libmi355rec_embed.so", "libmi355rec_embed_batch.so", "libmi355rec_embed_half.so", "libmi355rec_embed_sets.so",
                  "libmi355rec_embed_stream.so", "libmi355rec_embed_cand.so"):
        assert other not in dyn, "the companions share nothing but the product library"


def test_null_arguments_are_refused(multi_lib_path):
    from spotify_recommender_amd import capi
    L = capi.embed_multi_lib()
    e = ctypes.c_void_p()
    table = (ctypes.c_float * 16)()
    for create in (L.mi355rec_embed_multi_create, L.mi355rec_embed_multi_create_device):
        assert create(None, table, 1, 16, capi.EMBED_STREAM_FP32, ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
        assert b"null argument" in L.mi355rec_embed_multi_last_error(None)
        assert create(ctypes.c_void_p(16), table, 1, 16, capi.EMBED_STREAM_FP32, None) == capi.ERR_INVALID_ARG   # (out is looked at first)
        assert create(ctypes.c_void_p(16), None, 1, 16, capi.EMBED_STREAM_FP32, ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
        assert b"null table or negative n" in L.mi355rec_embed_multi_last_error(None)
        assert create(ctypes.c_void_p(16), table, -1, 16, capi.EMBED_STREAM_FP32, ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
    assert L.mi355rec_embed_multi_enqueue_query(None, None, None, None) == capi.ERR_INVALID_ARG
    assert b"null table" in L.mi355rec_embed_multi_last_error(None)
    assert L.mi355rec_embed_multi_info(None, None) == capi.ERR_INVALID_ARG
    L.mi355rec_embed_multi_destroy(None)


def test_kernels_are_gfx950_scratch_free_and_on_budget(multi_lib_path, golden_dir):
    from spotify_recommender_amd import build
    golden = json.loads((golden_dir / "embed_multi_kernel_budgets.json").read_text())
    assert build.check_no_scratch(multi_lib_path) == len(golden)
    meta = {k["name"]: k for k in build.kernel_metadata(multi_lib_path)}
    assert sorted(meta) == sorted(g["name"] for g in golden), "a kernel came or went"
    labels = sorted(g["label"] for g in golden)
    scans = [x for x in labels if x.startswith("embed_multi_scan_kernel<")]
    assert scans == sorted(f"embed_multi_scan_kernel<{s}, {d}>" for d in (16, 32, 64, 128) for s in ("f32", "fp16", "bf16")), scans
    # the set is exactly: the twelve scans, the finish, and what the shared headers instantiate (prepare and merge among them)
    assert sorted(set(labels) - set(scans)) == sorted(("embed_multi_finish_kernel",) + SHARED), labels
    assert len(labels) == len(set(labels)) == 12 + 1 + len(SHARED)
    design = (golden_dir.parents[1] / "DESIGN.md").read_text()
    section = design[design.index("### 5.4.30"):]
    section = section[: section.index("\n## ")] if "\n## " in section else section
    for g in golden:
        k = meta[g["name"]]
        assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] <= 65536, (g["label"], k)
        assert (k["vgpr"], k["lds"]) == (g["vgpr"], g["lds"]), (g["label"], k)
        row = f"| `{g['label']}` | {g['vgpr']} | {g['lds']} |"
        assert row in section, f"DESIGN.md §5.4.30 does not carry the row {row}"


def test_the_shared_kernels_are_the_stream_librarys(multi_lib_path, golden_dir):
    """The same kernels compiled into this library come out at the figures the stream library records for them."""
    mine = {g["label"]: (g["vgpr"], g["lds"]) for g in json.loads((golden_dir / "embed_multi_kernel_budgets.json").read_text())}
    stream = {g["label"]: (g["vgpr"], g["lds"]) for g in json.loads((golden_dir / "embed_stream_kernel_budgets.json").read_text())}
    for shared in SHARED:
        assert mine[shared] == stream[shared], shared


def test_the_chunk_width_is_what_the_design_says(golden_dir):
    """kEmbedMultiPass, the width DESIGN.md §5.4.30 argues for and the scan's launch bounds, as the sources state them."""
    root = golden_dir.parents[1]
    kernels = (root / "spotify_recommender_amd" / "csrc" / "embed_multi.hip.h").read_text()
    width = int(re.search(r"#define MI355REC_EMBED_MULTI_PASS (\d+)", kernels).group(1))
    assert width >= 1 and width & (width - 1) == 0 and 32 % width == 0
    design = (root / "DESIGN.md").read_text()
    section = design[design.index("### 5.4.30"):]
    assert f"P = {width}" in section
    assert kernels.count("__launch_bounds__(kEmbedBlock, 4)") == 1 and "asm" not in re.sub(r"//.*", "", kernels)
