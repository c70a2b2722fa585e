"""The companion library libmi355rec_embed.so (include/mi355rec_embed.h) as a build product, without a GPU: it builds for
gfx950, exports exactly what its header declares and capi.EMBED_SIGNATURES binds all of it (and none of it sits in
capi.SIGNATURES), no kernel reserves scratch, and every kernel's VGPRs and LDS are the figures of DESIGN.md §5.4.21 as
recorded in tests/golden/embed_kernel_budgets.json.  (That libmi355rec.so still holds its sixty kernels at their figures
is what the unchanged tests/test_kernel_metadata.py shows.)"""
import ctypes
import json
import re
import subprocess

import pytest

from tests.test_capi_cpu import declared_symbols


@pytest.fixture(scope="module")
def embed_lib_path():
    from spotify_recommender_amd import build
    return build.build_embed()


def test_exports_are_the_header_and_the_bindings(embed_lib_path, golden_dir):
    from spotify_recommender_amd import build, capi
    root = golden_dir.parents[1]
    declared = [s for s in declared_symbols(root, "mi355rec_embed.h") if s.startswith("mi355rec_embed_")]
    assert len(declared) == 8, declared
    syms = subprocess.run([str(build.LLVM_BIN / "llvm-readelf"), "--dyn-syms", "-W", str(embed_lib_path)], capture_output=True, text=True,
                          check=True).stdout
    # (Num: Value Size Type Bind Vis Ndx Name; Ndx UND = imported from libmi355rec.so, not exported)
    exported = sorted({f[7].split("@")[0] for f in (line.split() for line in syms.splitlines())
                       if len(f) >= 8 and f[6] != "UND" and re.match(r"mi355rec_", f[7])})
    assert exported == declared, "the library exports something its header does not declare, or the reverse"
    assert set(capi.EMBED_SIGNATURES) == set(declared)
    assert not set(capi.EMBED_SIGNATURES) & set(capi.SIGNATURES), "the companion's names belong to the second table only"
    L = capi.embed_lib()
    for name, (_, argtypes) in capi.EMBED_SIGNATURES.items():
        assert getattr(L, name).argtypes == argtypes, name
    assert ctypes.sizeof(capi.EmbedQuery) == 72 and ctypes.sizeof(capi.EmbedResult) == 32 and ctypes.sizeof(capi.EmbedInfo) == 56
    assert capi.EmbedQuery.audio_row.offset == 40 and capi.EmbedQuery.w_embed.offset == 68
    # the two accessors the companion needs are the product library's, declared in its own header
    for name in ("mi355rec_sharded_shard_handle", "mi355rec_sharded_host_rows"):
        assert name in capi.SIGNATURES and name in declared_symbols(root, "mi355rec_diag.h")


def test_it_links_against_the_product_library_beside_it(embed_lib_path):
    from spotify_recommender_amd import build
    dyn = subprocess.run([str(build.LLVM_BIN / "llvm-readelf"), "-d", str(embed_lib_path)], capture_output=True, text=True, check=True).stdout
    assert "libmi355rec.so" in dyn and "$ORIGIN" in dyn


def test_kernels_are_gfx950_scratch_free_and_on_budget(embed_lib_path, golden_dir):
    from spotify_recommender_amd import build
    assert build.check_no_scratch(embed_lib_path) == 7
    meta = {k["name"]: k for k in build.kernel_metadata(embed_lib_path)}
    golden = json.loads((golden_dir / "embed_kernel_budgets.json").read_text())
    assert sorted(meta) == sorted(g["name"] for g in golden), "a kernel came or went"
    design = (golden_dir.parents[1] / "DESIGN.md").read_text()
    section = design[design.index("### 5.4.21"):]
    section = section[: section.index("\n## ")] if "\n## " in section else section
    for g in golden:
        k = meta[g["name"]]
        assert (k["vgpr"], k["lds"], k["scratch"]) == (g["vgpr"], g["lds"], 0), (g["label"], k)
        assert k["vgpr"] <= 128, "two 512-thread workgroups per CU need at most 128 VGPRs"
        row = f"| `{g['label']}` | {g['vgpr']} | {g['lds']} |"
        assert row in section, f"DESIGN.md §5.4.21 does not carry the row {row}"
