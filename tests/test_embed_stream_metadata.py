"""The fifth companion library libmi355rec_embed_stream.so (include/mi355rec_embed_stream.h) as a build product, without a
GPU: it builds for gfx950, exports exactly what its header declares, capi.EMBED_STREAM_SIGNATURES binds all of it and shares
no name with the other five tables, it links libmi355rec.so through $ORIGIN and no other companion, NULL arguments are
refused, no kernel reserves scratch or leaves the budget of two 512-thread workgroups per CU (128 VGPRs, 64 KiB LDS), and
every kernel's figures are the record in tests/golden/embed_stream_kernel_budgets.json, whose rows stand in DESIGN.md
§5.4.27.  (That the other libraries did not move under the borrowed-table flag of the shared host path is what the
unchanged metadata tests of each show.)"""
import ctypes
import itertools
import json
import re
import subprocess

import pytest

from tests.test_capi_cpu import declared_symbols

ENTRY_POINTS = ("create", "create_device", "destroy", "last_error", "info", "enqueue_query", "enqueue_users")


@pytest.fixture(scope="module")
def stream_lib_path():
    from spotify_recommender_amd import build
    return build.build_embed_stream()


def test_exports_are_the_header_and_the_bindings(stream_lib_path, golden_dir):
    from spotify_recommender_amd import build, capi
    root = golden_dir.parents[1]
    declared = declared_symbols(root, "mi355rec_embed_stream.h")
    assert declared == sorted(f"mi355rec_embed_stream_{x}" for x in ENTRY_POINTS)
    syms = subprocess.run([str(build.LLVM_BIN / "llvm-readelf"), "--dyn-syms", "-W", str(stream_lib_path)], capture_output=True, text=True,
                          check=True).stdout
    # (Num: Value Size Type Bind Vis Ndx Name; Ndx UND = imported from libmi355rec.so, not exported)
    exported = sorted({f[7].split("@")[0] for f in (line.split() for line in syms.splitlines())
                       if len(f) >= 8 and f[6] != "UND" and re.match(r"mi355rec_", f[7])})
    assert exported == declared, "the library exports something its header does not declare, or the reverse"
    imported = sorted({f[7].split("@")[0] for f in (line.split() for line in syms.splitlines())
                       if len(f) >= 8 and f[6] == "UND" and re.match(r"mi355rec_", f[7])})
    assert imported == ["mi355rec_enqueue_scores", "mi355rec_last_error", "mi355rec_stats"], "what the library asks of the product library"
    assert set(capi.EMBED_STREAM_SIGNATURES) == set(declared)
    tables = [capi.SIGNATURES, capi.EMBED_SIGNATURES, capi.EMBED_BATCH_SIGNATURES, capi.EMBED_HALF_SIGNATURES, capi.EMBED_SETS_SIGNATURES,
              capi.EMBED_STREAM_SIGNATURES]
    for a, b in itertools.combinations(tables, 2):
        assert not set(a) & set(b), "the six tables are pairwise disjoint"
    L = capi.embed_stream_lib()
    for name, (_, argtypes) in capi.EMBED_STREAM_SIGNATURES.items():
        assert getattr(L, name).argtypes == argtypes, name


def test_struct_sizes_and_offsets():
    from spotify_recommender_amd import capi
    Q, U, R, I = capi.EmbedStreamQuery, capi.EmbedStreamUsers, capi.EmbedStreamResult, capi.EmbedStreamInfo
    assert ctypes.sizeof(Q) == 64
    assert [getattr(Q, f).offset for f, _ in Q._fields_] == [0, 4, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60]
    assert ctypes.sizeof(U) == 48
    assert [getattr(U, f).offset for f, _ in U._fields_] == [0, 4, 8, 16, 24, 28, 32, 36, 40, 44]
    assert ctypes.sizeof(R) == 32 and [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 16, 24]
    assert ctypes.sizeof(I) == 80
    assert [getattr(I, f).offset for f, _ in I._fields_] == [0, 4, 8, 16, 24, 28, 32, 36, 40, 48, 56, 64, 72, 76]
    assert capi.EMBED_STREAM_FP32 == -1 and (capi.EMBED_HALF_FP16, capi.EMBED_HALF_BF16) == (0, 1)
    assert (capi.EMBED_STREAM_MAX_EXCLUDE, capi.EMBED_STREAM_MAX_USERS, capi.EMBED_STREAM_MAX_USERS_TOPN) == (1024, 1024, 128)


def test_it_links_against_the_product_library_beside_it(stream_lib_path):
    from spotify_recommender_amd import build
    dyn = subprocess.run([str(build.LLVM_BIN / "llvm-readelf"), "-d", str(stream_lib_path)], capture_output=True, text=True, check=True).stdout
    assert "libmi355rec.so" in dyn and "$ORIGIN" in dyn
    for other in ("libmi355rec_embed.so", "libmi355rec_embed_batch.so", "libmi355rec_embed_half.so", "libmi355rec_embed_sets.so"):
        assert other not in dyn, "the companions share nothing but the product library"


def test_null_arguments_are_refused(stream_lib_path):
    from spotify_recommender_amd import capi
    L = capi.embed_stream_lib()
    e = ctypes.c_void_p()
    table = (ctypes.c_float * 16)()
    for create in (L.mi355rec_embed_stream_create, L.mi355rec_embed_stream_create_device):
        assert create(None, table, 1, 16, capi.EMBED_STREAM_FP32, ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
        assert b"null argument" in L.mi355rec_embed_stream_last_error(None)
        assert create(ctypes.c_void_p(16), table, 1, 16, capi.EMBED_STREAM_FP32, None) == capi.ERR_INVALID_ARG   # (out is looked at first)
        assert create(ctypes.c_void_p(16), None, 1, 16, capi.EMBED_STREAM_FP32, ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
        assert b"null table or negative n" in L.mi355rec_embed_stream_last_error(None)
        assert create(ctypes.c_void_p(16), table, -1, 16, capi.EMBED_STREAM_FP32, ctypes.byref(e)) == capi.ERR_INVALID_ARG and not e
    assert L.mi355rec_embed_stream_enqueue_query(None, None, None, None) == capi.ERR_INVALID_ARG
    assert L.mi355rec_embed_stream_enqueue_users(None, None, None, None) == capi.ERR_INVALID_ARG
    assert b"null table" in L.mi355rec_embed_stream_last_error(None)
    assert L.mi355rec_embed_stream_info(None, None) == capi.ERR_INVALID_ARG
    L.mi355rec_embed_stream_destroy(None)


def test_kernels_are_gfx950_scratch_free_and_on_budget(stream_lib_path, golden_dir):
    from spotify_recommender_amd import build
    golden = json.loads((golden_dir / "embed_stream_kernel_budgets.json").read_text())
    assert build.check_no_scratch(stream_lib_path) == len(golden)
    meta = {k["name"]: k for k in build.kernel_metadata(stream_lib_path)}
    assert sorted(meta) == sorted(g["name"] for g in golden), "a kernel came or went"
    labels = sorted(g["label"] for g in golden)
    scans = [x for x in labels if x.startswith("embed_stream_scan_kernel<")]
    assert scans == sorted(f"embed_stream_scan_kernel<{s}, {d}>" for d in (16, 32, 64, 128) for s in ("f32", "fp16", "bf16")), scans
    assert [x for x in labels if x.startswith("embed_batch_scan_kernel<")] == sorted(f"embed_batch_scan_kernel<{d}, 8>" for d in (16, 32, 64, 128))
    assert {"embed_stream_prepare_kernel", "embed_stream_finish_kernel", "merge_kernel"} <= set(labels)
    design = (golden_dir.parents[1] / "DESIGN.md").read_text()
    section = design[design.index("### 5.4.27"):]
    section = section[: section.index("\n## ")] if "\n## " in section else section
    for g in golden:
        k = meta[g["name"]]
        assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] <= 65536, (g["label"], k)
        assert (k["vgpr"], k["lds"]) == (g["vgpr"], g["lds"]), (g["label"], k)
        row = f"| `{g['label']}` | {g['vgpr']} | {g['lds']} |"
        assert row in section, f"DESIGN.md §5.4.27 does not carry the row {row}"


def test_the_scans_are_the_other_libraries_scans(stream_lib_path, golden_dir):
    """The same bodies compiled into this library come out at the figures the other libraries record for them: the fp32 and
    half single-user scans (embed_scan_kernel, embed_half_scan_kernel), the batch scan and the merge."""
    mine = {g["label"]: (g["vgpr"], g["lds"]) for g in json.loads((golden_dir / "embed_stream_kernel_budgets.json").read_text())}
    def record(name):
        return {g["label"]: (g["vgpr"], g["lds"]) for g in json.loads((golden_dir / name).read_text())}

    batch, half, single = record("embed_batch_kernel_budgets.json"), record("embed_half_kernel_budgets.json"), record("embed_kernel_budgets.json")
    for d in (16, 32, 64, 128):
        assert mine[f"embed_batch_scan_kernel<{d}, 8>"] == batch[f"embed_batch_scan_kernel<{d}, 8>"], d
        assert mine[f"embed_stream_scan_kernel<f32, {d}>"] == single[f"embed_scan_kernel<{d}>"], d
        for s in ("fp16", "bf16"):
            assert mine[f"embed_stream_scan_kernel<{s}, {d}>"] == half[f"embed_half_scan_kernel<{d}, {s}>"], (d, s)
    for shared in ("merge_kernel", "embed_user_kernel", "embed_probe_kernel", "embed_half_user_kernel"):
        assert mine[shared] == half[shared], shared
