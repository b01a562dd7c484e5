"""The device PNG encoder's host side (cfen_vit_dehazing_amd/png.py) and its numpy restatement (tests/png_ref.py), without a GPU: the candidate
Huffman tables, the stream format, the container, the size bounds that follow from the format, and the option conflicts of --gpu_png.

Size bounds.  A strip of n filtered bytes costs at most n + 10 bytes (stored block: 5 bytes of framing; the empty stored block after it: 5), a dynamic
block is taken only when strictly smaller; header, closing block and Adler-32 add 2 + 5 + 4.  So stream <= filtered bytes + 10 S + 11 for S strips.
The tightest table codes residuals 0, +1 and -1 in at most 3 bits, so an image whose filtered bytes are all of those costs at most 3/8 of its bytes
plus the per-strip block header and framing: under 50 % of the raw pixels once a strip is a few kilobytes."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import png_ref
from cfen_vit_dehazing_amd import png
from cfen_vit_dehazing_amd.options.test_options import TestOptions


def _kraft(lengths):
    return sum(1 << (png.MAX_BITS - l) for l in lengths if l)


def test_sixteen_tables_each_complete_and_within_15_bits():
    tabs = png.tables()
    assert len(tabs) == len(png.SCALES) == 16
    for t in tabs:
        assert len(t.lengths) == len(t.codes) == 257
        assert all(1 <= l <= png.MAX_BITS for l in t.lengths)
        assert _kraft(t.lengths) == 1 << png.MAX_BITS                       # complete: Kraft sum exactly 1
        assert t.header_bits <= 32 * png.TABLE_HEADER_WORDS
        # canonical and prefix-free: the un-reversed codes, sorted by (length, symbol), count up
        codes = png.canonical_codes(t.lengths)
        assert [png.bit_reverse(c, l) for c, l in zip(codes, t.lengths)] == t.codes
        order = sorted(range(257), key=lambda s: (t.lengths[s], s))
        as_fraction = [codes[s] << (png.MAX_BITS - t.lengths[s]) for s in order]
        assert all(b - a == 1 << (png.MAX_BITS - t.lengths[s]) for a, b, s in zip(as_fraction, as_fraction[1:], order))


def test_tightest_table_codes_small_residuals_in_three_bits():
    t = png.tables()[0]
    assert max(t.lengths[0], t.lengths[1], t.lengths[255]) <= 3


def test_table_blob_layout():
    blob = png.table_blob()
    assert blob.shape == (16, png.TABLE_WORDS) and blob.dtype == np.uint32
    for row, t in zip(blob, png.tables()):
        assert row[0] == t.header_bits
        assert list(row[png.TABLE_CODES_AT:png.TABLE_CODES_AT + 257] >> 16) == t.lengths
        assert list(row[png.TABLE_CODES_AT:png.TABLE_CODES_AT + 257] & 0xFFFF) == t.codes
        assert not row[png.TABLE_CODES_AT + 257:].any()


@pytest.mark.parametrize("k", range(16))
def test_table_header_and_coded_sample_inflate(k):
    """a raw deflate stream made of this table's header, a coded sample holding every symbol, and the closing stored block"""
    t = png.tables()[k]
    rs = np.random.RandomState(k)
    sample = np.concatenate([np.arange(256), rs.randint(0, 256, 1000), np.zeros(50, dtype=np.int64)]).astype(np.uint8)
    bits = png._Bits()
    bits.put(sum(w << (32 * i) for i, w in enumerate(t.header_words)), t.header_bits)
    for s in list(sample) + [256]:
        bits.put(t.codes[s], t.lengths[s])
    bits.put(0, 3)                                             # the empty stored block, non-final
    nbytes = (bits.n + 7) // 8
    raw = bits.acc.to_bytes(nbytes, "little") + b"\x00\x00\xff\xff" + b"\x01\x00\x00\xff\xff"
    d = zlib.decompressobj(wbits=-15)
    assert d.decompress(raw) == sample.tobytes()
    assert d.eof and d.unused_data == b""


@pytest.mark.parametrize("name", list(png_ref.SMALL_CASES))
def test_restated_stream_inflates_to_the_filtered_scanlines_and_pil_reads_the_file(name):
    img = png_ref.SMALL_CASES[name]()
    H, W, _ = img.shape
    blocks = []
    stream = png_ref.stream(img, blocks)
    R, S, rowb, strip_bytes, out_stride = png.geometry(H, W)
    assert len(blocks) == S and len(stream) <= out_stride
    assert stream[:2] == b"\x78\x01"
    assert zlib.decompress(stream) == png_ref.filtered_scanlines(img).tobytes()
    assert len(stream) <= H * rowb + 10 * S + 11
    back = Image.open(io.BytesIO(png.assemble(stream, H, W)))
    assert back.mode == "RGB" and back.size == (W, H)
    assert np.array_equal(np.array(back), img)


def test_geometry_of_the_named_cases():
    assert png.geometry(3, 10922)[:3] == (1, 3, 32767)                     # the widest image: one row per strip
    assert png.geometry(100, 300)[:2] == (36, 3)                           # 36 + 36 + 28 rows
    assert png.geometry(512, 512)[:2] == (21, 25)
    assert png.geometry(2160, 3840)[:2] == (2, 1080)
    assert png.geometry(1, 1)[:4] == (8192, 1, 4, 32)


def test_filter_choice_ties_go_to_the_lowest_type():
    lines = png_ref.filtered_scanlines(np.zeros((4, 5, 3), dtype=np.uint8))
    assert not lines.any()                                                 # every filter scores 0: None
    lines = png_ref.filtered_scanlines(png_ref.ramp(8, 64))
    assert lines[0, 0] == 1 and set(lines[1:, 0]) == {2}                   # Sub on row 0 (Sub = Average-free minimum), Up below


def test_noise_is_stored_and_within_the_framing_bound():
    img = png_ref.noise(64, 80, 1)
    blocks = []
    stream = png_ref.stream(img, blocks)
    R, S, rowb, _, _ = png.geometry(64, 80)
    assert set(blocks) == {-1}
    assert len(stream) == 64 * rowb + 10 * S + 11
    assert len(stream) <= img.size + 64 + 10 * S + 11                      # raw pixels + filter bytes + framing


def test_ramp_is_under_half_of_raw():
    img = png_ref.ramp(96, 160)
    assert len(png_ref.stream(img)) < img.size // 2


def test_row_limit():
    assert png.geometry(1, 10922)[2] == 32767
    with pytest.raises(png.RowTooLong):
        png.geometry(1, 10923)
    with pytest.raises(ValueError):
        png.geometry(0, 4)


def _parse(tmp_path, *extra):
    argv = ["--dataroot", str(tmp_path), "--checkpoints_dir", str(tmp_path / "ck"), "--results_dir", str(tmp_path / "res"), "--gpu_ids", "-1"]
    return TestOptions().parse(argv + list(extra))


def test_gpu_png_option_and_its_conflicts(tmp_path, capsys):
    assert _parse(tmp_path).gpu_png is False
    assert "gpu_png:" not in capsys.readouterr().out                       # a run without the flag prints what it always did
    assert _parse(tmp_path, "--gpu_png").gpu_png is True
    assert _parse(tmp_path, "--gpu_png", "--in_flight", "4", "--writers", "3").gpu_png is True
    with pytest.raises(ValueError, match="writer_procs"):
        _parse(tmp_path, "--gpu_png", "--in_flight", "4", "--writer_procs", "2")
    with pytest.raises(ValueError, match="png_compress_level"):
        _parse(tmp_path, "--gpu_png", "--png_compress_level", "1")
