"""CPU: ii2_count_ranges / TermCounts are wired through every layer - header, export map, binding, Makefile, host mirror and
the Python faces - and the counting kernels keep to their rule that no workgroup waits for another."""
import ctypes as C
import fnmatch
import os
import re

from inverted_index_2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "inverted_index_2_amd", "csrc")


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "ii2.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(ii2_[a-z0-9_]+)\s*\(", text))


def _built():
    from inverted_index_2_amd import host
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(host.HOST_LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()


def test_count_ranges_is_declared_exported_and_bound():
    assert "ii2_count_ranges" in _header_symbols()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "exports.map")).read(), flags=re.S)
    exported = re.search(r"global:(.*?);\s*local:", text, flags=re.S).group(1)
    assert any(fnmatch.fnmatchcase("ii2_count_ranges", pat.strip()) for pat in exported.split(";") if pat.strip())
    assert "ii2_count_ranges" in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES["ii2_count_ranges"]
    assert res is C.c_int and len(args) == 11


def test_count_stats_layout():
    # four u64 and one u32, padded to 40 bytes, as the header lays it out
    assert [f[0] for f in _lib.CountStats._fields_] == ["n_lists", "n_blocks", "n_decoded", "n_hits", "n_windows"]
    assert C.sizeof(_lib.CountStats) == 40
    header = open(os.path.join(ROOT, "include", "ii2.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*ii2_count_stats;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == ["n_lists", "n_blocks", "n_decoded", "n_hits", "n_windows"]


def test_count_ranges_object_is_in_the_makefile():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(line for line in mk.splitlines() if line.startswith("OBJS"))
    assert "build/count_ranges.o" in objs.split()


def test_count_kernels_have_no_inter_workgroup_waits():
    src = open(os.path.join(CSRC, "count_ranges.hip")).read()
    assert "lookback.h" not in src and "ii2_lookback_launch" not in src
    for k in ("k_cr_mark", "k_cr_count", "cr_walk<", "seg_or"):
        assert k in src, k
    # the walk and the block decode are shared with the other readers of a marked set, not copied into the kernel files
    walk = open(os.path.join(CSRC, "cr_walk.h")).read()
    assert "decode_block_wave4" in walk and "um_range_of(" in walk and "lookback.h" not in walk
    for name in ("count_ranges.hip", "explain_ranges.hip", "histogram.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert "um_range_of(" not in text and "cr_walk<" in text, name
    # the segmented OR is shared with the block-wise union, not copied
    assert "uint32_t seg_or(" not in src
    assert "uint32_t seg_or(" not in open(os.path.join(CSRC, "union_many.hip")).read()


def test_null_context_is_einval():
    _built()
    assert _lib.load().ii2_count_ranges(None, 0, None, None, None, None, 0, None, None, 0, None) == -1      # II2_EINVAL


def test_host_library_exports_term_counts():
    from inverted_index_2_amd import host
    _built()
    C.CDLL(_lib.LIB_PATH)        # dependency first
    assert hasattr(C.CDLL(host.HOST_LIB_PATH), "ii2h_term_counts")


def test_python_faces():
    from inverted_index_2_amd import Context, host
    assert callable(getattr(Context, "count_ranges", None))
    assert callable(getattr(host.InvertedIndex, "term_counts", None))
