"""CPU: the case table of tests/test_gpu_caller_stream.py against include/h2agg.h — every declaration of an entry point whose
name says that it takes device buffers or queues (h2agg_*_device*, h2agg_*_async*) has a stream case, classed `queued` or
`synchronous`, so a new one cannot arrive without — and every case's decoy is a real decoy: from the references alone, its
expected output differs from the true input's."""
import os
import re

import pytest

import __graft_entry__ as entry
from tests import test_gpu_caller_stream as M

HEADER = os.path.join(entry.ROOT, "include", "h2agg.h")


def declared_device_entry_points():
    """the names declared (a return type in front, an argument list behind), not the ones a comment mentions"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    names = re.findall(r"\b(?:int|void|size_t|const\s+char\s*\*)\s+(h2agg_\w+)\s*\(", text)
    return {n for n in names if re.fullmatch(r"h2agg_\w*(_device|_async)\w*", n)}


def test_the_header_pattern_finds_the_declarations():
    found = declared_device_entry_points()
    assert "h2agg_fr_fft_device" in found and "h2agg_g1_msm_device_batch_async" in found and "h2agg_g1_msm_device" in found
    assert "h2agg_fr_fft" not in found and "h2agg_bases_generate" not in found


def test_every_device_buffer_entry_point_has_a_stream_case():
    assert declared_device_entry_points() == set(M.CASES)
    for name, (kind, variants) in M.CASES.items():
        assert kind in (M.QUEUED, M.SYNCHRONOUS) and variants, name
    assert not set(M.EXTRA_SYNCHRONOUS) & set(M.CASES)


def test_the_classes_are_the_headers():
    """queued = the header says "queued on the context's stream" / "asynchronous"; synchronous = results go to the host"""
    queued = {n for n, (kind, _v) in M.CASES.items() if kind == M.QUEUED}
    assert queued == {"h2agg_fr_fft_device", "h2agg_fr_poly_divide_device", "h2agg_fr_batch_invert_device",
                      "h2agg_fr_grand_product_device", "h2agg_permutation_product_device", "h2agg_lookup_product_device",
                      "h2agg_lookup_permute_device", "h2agg_fr_columns_compress_device", "h2agg_vk_expressions_eval_device",
                      "h2agg_quotient_device", "h2agg_g1_msm_device_async", "h2agg_g1_msm_device_batch_async"}


@pytest.mark.parametrize("name,variant", [(n, v) for n, v, _b in M.every_work()])
def test_the_decoy_is_a_decoy(name, variant):
    build = dict(((n, v), b) for n, v, b in M.every_work())[(name, variant)]
    w = build()
    assert w.true_in != w.decoy_in and len(w.true_in) == len(w.decoy_in)
    assert w.want != w.want_decoy
    assert len(w.want) == len(w.want_decoy)
    if w.out_bytes and w.raw:
        assert len(w.want) == w.out_bytes
