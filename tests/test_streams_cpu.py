"""Every device entry point of include/polyhip.h has a case in tests/test_streams_gpu.py: the header is parsed for the
functions that take a polyhip_stream_t, plus the three _dev read-backs that take none, and each must be named in that
module's COVERED list (no GPU needed: the module is only imported).  A new device entry point cannot arrive without a
stream case."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

STREAMLESS_READBACKS = ["polyhip_mash_index_format_dev", "polyhip_mash_index_build_info_dev",
                        "polyhip_mash_shared_counts_mode_dev"]


def _header_functions():
    """[(name, parameter text)] of every function declared in the header"""
    text = open(os.path.join(ROOT, "include", "polyhip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.findall(r"\b(polyhip_\w+)\s*\(([^()]*)\)\s*;", text)


def test_every_device_entry_point_has_a_stream_case():
    import test_streams_gpu as tsg
    funcs = _header_functions()
    names = [n for n, _ in funcs]
    assert len(names) > 80 and "polyhip_abi_version" in names, "the header was not parsed"
    streamed = [n for n, params in funcs if "polyhip_stream_t" in params]
    assert len(streamed) >= 31 and "polyhip_mash_sketch_batch_dev" in streamed and "polyhip_allgatherv_dev" in streamed
    for n in STREAMLESS_READBACKS:
        assert n in names and n not in streamed
    missing = [n for n in streamed + STREAMLESS_READBACKS if n not in tsg.COVERED]
    assert not missing, f"device entry points without a case in tests/test_streams_gpu.py: {missing}"
    unknown = [n for n in tsg.COVERED if n not in names]
    assert not unknown, f"COVERED names functions the header does not declare: {unknown}"
    assert len(set(tsg.COVERED)) == len(tsg.COVERED)
    # every other _dev function is reached through a stream parameter
    assert not [n for n in names if n.endswith("_dev") and n not in tsg.COVERED]
    assert set(tsg.SYNCHRONISING) <= set(streamed)


def test_every_covered_entry_point_is_called_by_the_module():
    """COVERED is not a list of good intentions: the wrapper of each entry in poly_amd is called in the test module"""
    import test_streams_gpu as tsg
    src = open(os.path.join(HERE, "test_streams_gpu.py")).read()
    wrapper = {
        "polyhip_mash_sketch_batch_dev": "sketch_batch_dev(", "polyhip_mash_index_format_dev": "index_item_bytes(",
        "polyhip_mash_index_build_info_dev": "index_build_info(", "polyhip_mash_shared_counts_mode_dev": "shared_counts_mode(",
        "polyhip_mash_index_part_spans": "index_part_spans(", "polyhip_mash_index_allgather_dev": "index_allgather(",
        "polyhip_sw_align_batch_dev": "sw_align_dev(", "polyhip_nw_align_batch_dev": "nw_align_dev(",
        "polyhip_fastq_pack_dev": "fastq", "polyhip_fasta_pack_dev": "fasta", "polyhip_bwt_create_dev": "bwt.new_dev(",
        "polyhip_bwt_transform_dev": "bwt.transform_dev(", "polyhip_bwt_count_dev": "bwt.count_dev(",
        "polyhip_bwt_locate_dev": "bwt.locate_dev(", "polyhip_bwt_extract_dev": "bwt.extract_dev(",
        "polyhip_allgather_sketches_dev": "allgather_sketches(", "polyhip_allgatherv_dev": "allgatherv(",
    }
    for n in tsg.COVERED:
        call = wrapper.get(n, n[len("polyhip_"):].replace("mash_", "", 1) + "(")
        assert call in src, f"{n}: no call of {call} in tests/test_streams_gpu.py"
