"""Motion-JPEG output path without a GPU: the test-side JPEG restatement (tests/mjpeg_ref.py) against an independent decoder (PIL /
libjpeg-turbo), the package's fixed JFIF headers against the restatement's, and the AVI container (mmgt_amd.video_out.write_avi) walked chunk
by chunk and read back through mmgt_amd.inputs.read_frames.  write_avi is fed PIL-made JPEGs here."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

from tests import mjpeg_ref as R

SIZES = [(64, 64), (40, 56), (17, 9)]                      # (H, W): on the MCU multiple, off it for 16 x 16, off it for 8 x 8 too


def _pil_jpeg(frame, quality=90, subsampling="4:2:0"):
    b = io.BytesIO()
    Image.fromarray(frame).save(b, "JPEG", quality=quality, subsampling={"4:2:0": 2, "4:4:4": 0}[subsampling], restart_marker_rows=1)
    return b.getvalue()


def _segments(jpeg, marker):
    """Bodies of the marker segments `marker` in the header part of a JPEG file."""
    out, i = [], 2
    while jpeg[i + 1] != 0xDA:
        n = int.from_bytes(jpeg[i + 2:i + 4], "big")
        if jpeg[i + 1] == marker:
            out.append(jpeg[i + 4:i + 2 + n])
        i += 2 + n
    return out


@pytest.mark.parametrize("subsampling", ["4:2:0", "4:4:4"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("quality", [1, 50, 90, 100])
def test_restatement_files_open_in_pil(subsampling, size, quality):
    H, W = size
    frame = R.smooth_frame(H, W, seed=H * W + quality)
    data = R.encode(frame, quality, subsampling)
    img = Image.open(io.BytesIO(data))
    img.load()
    assert img.format == "JPEG" and img.size == (W, H) and img.mode == "RGB"
    # the decode is a picture of the source: within 1 dB of what PIL's own encoder keeps at the same settings (printed, loose: the tight
    # comparison with margins is the GPU test's)
    mine, pil = R.psnr(np.asarray(img), frame), R.psnr(np.asarray(Image.open(io.BytesIO(_pil_jpeg(frame, quality, subsampling)))), frame)
    print(f"{subsampling} {H}x{W} q{quality}: {len(data)} B, PSNR {mine:.2f} dB (PIL's encoder {pil:.2f} dB)")
    assert mine > pil - 1.0


def test_restatement_noise_at_quality_100_decodes():
    """Uniform noise at quality 100: long codes, many 0xFF bytes to stuff."""
    frame = R.noise_frame(48, 72, 5)
    for ss in ("4:2:0", "4:4:4"):
        data = R.encode(frame, 100, ss)
        assert data.count(b"\xff\x00") > 0
        img = Image.open(io.BytesIO(data))
        img.load()
        assert img.size == (72, 48)
    assert R.psnr(np.asarray(img), frame) > 40.0           # 4:4:4 at quality 100 keeps noise nearly intact


def test_tables_are_the_standard_ones():
    """The restatement's and the package's quantiser / Huffman tables are what libjpeg writes for the same quality (both are T.81 Annex K)."""
    from mmgt_amd import video_out
    frame = R.smooth_frame(32, 32, 0)
    for q in (1, 25, 50, 75, 90, 100):
        pil = _pil_jpeg(frame, q)
        assert _segments(R.headers(32, 32, q, "4:2:0"), 0xDB) == _segments(pil, 0xDB)
        assert video_out.jfif_headers(32, 32, q, "4:2:0") == R.headers(32, 32, q, "4:2:0")
    assert b"".join(b[0:] for b in _segments(R.headers(32, 32, 50, "4:2:0"), 0xC4)) == b"".join(_segments(_pil_jpeg(frame, 50), 0xC4))
    for ss, (H, W) in (("4:4:4", (17, 9)), ("4:2:0", (40, 56))):
        assert video_out.jfif_headers(W, H, 90, ss) == R.headers(W, H, 90, ss)


def test_bad_arguments_raise_the_librarys_error():
    from mmgt_amd import hip, video_out
    with pytest.raises(RuntimeError, match="quality"):
        hip.jpeg_qtables(0)
    with pytest.raises(RuntimeError, match="quality"):
        video_out.jfif_headers(64, 64, 101)
    with pytest.raises(RuntimeError, match="subsampling"):
        hip.jpeg_segment_stride(64, "4:2:2")


# ---- the container -----------------------------------------------------------------------------------------------------------------------------
def _walk(buf, start, end):
    pos = start
    while pos < end:
        cc, size = buf[pos:pos + 4], struct.unpack("<I", buf[pos + 4:pos + 8])[0]
        assert pos + 8 + size <= end, f"chunk {cc} at {pos} runs past its parent"
        yield cc, pos, pos + 8, size
        pos += 8 + size + (size & 1)
        assert pos % 2 == 0, "chunks start on even offsets"
    assert pos == end, "parent size is not the sum of its (padded) children"


def _parse_avi(buf):
    assert buf[:4] == b"RIFF" and buf[8:12] == b"AVI " and struct.unpack("<I", buf[4:8])[0] == len(buf) - 8
    top = {}
    for cc, pos, body, size in _walk(buf, 12, len(buf)):
        key = buf[body:body + 4] if cc == b"LIST" else cc
        assert key not in top
        top[key] = (pos, body, size)
    assert list(top) == [b"hdrl", b"movi", b"idx1"]
    info = {"streams": []}
    _, body, size = top[b"hdrl"]
    for cc, pos, b2, s2 in _walk(buf, body + 4, body + size):
        if cc == b"avih":
            assert s2 == 56
            info["avih"] = struct.unpack("<14I", buf[b2:b2 + 56])
        else:
            assert cc == b"LIST" and buf[b2:b2 + 4] == b"strl"
            st = {c3: buf[b3:b3 + s3] for c3, _, b3, s3 in _walk(buf, b2 + 4, b2 + s2)}
            assert set(st) == {b"strh", b"strf"} and len(st[b"strh"]) == 56
            info["streams"].append(st)
    movi_pos, movi_body, movi_size = top[b"movi"]
    info["chunks"] = [(cc, b2, s2) for cc, _, b2, s2 in _walk(buf, movi_body + 4, movi_body + movi_size)]
    _, ib, isz = top[b"idx1"]
    assert isz % 16 == 0
    info["index"] = [struct.unpack("<4sIII", buf[ib + 16 * k:ib + 16 * k + 16]) for k in range(isz // 16)]
    info["movi_fourcc_at"] = movi_body
    return info


@pytest.mark.parametrize("with_audio", [False, True])
def test_write_avi_container_fields_and_read_back(tmp_path, with_audio):
    from mmgt_amd import inputs, video_out
    H, W, n, fps, rate = 40, 56, 7, 25, 16000
    frames = [R.smooth_frame(H, W, seed=k) for k in range(n)]
    jpegs = [_pil_jpeg(f, 90 - k) for k, f in enumerate(frames)]                  # different qualities: odd and even sizes both occur
    assert {len(j) & 1 for j in jpegs} == {0, 1}
    rng = np.random.default_rng(7)
    pcm = rng.integers(-32768, 32767, (int(rate * n / fps) + 123, 2), dtype=np.int16) if with_audio else None
    path = tmp_path / "clip.avi"
    size = video_out.write_avi(str(path), jpegs, W, H, fps, audio=(pcm, rate) if with_audio else None)
    buf = path.read_bytes()
    assert size == len(buf)
    info = _parse_avi(buf)

    usec, _, _, flags, total, _, streams, sugg, w, h = info["avih"][:10]
    assert (usec, total, streams, w, h) == (40000, n, 2 if with_audio else 1, W, H) and flags & 0x10 and sugg >= max(map(len, jpegs))
    v = info["streams"][0]
    assert v[b"strh"][:8] == b"vidsMJPG"
    scale, vrate, _, length = struct.unpack("<4I", v[b"strh"][20:36])
    assert vrate / scale == fps and length == n
    bi = struct.unpack("<IiiHH4sIiiII", v[b"strf"])
    assert bi[:6] == (40, W, H, 1, 24, b"MJPG")
    if with_audio:
        a = info["streams"][1]
        assert a[b"strh"][:4] == b"auds"
        scale, arate, _, length = struct.unpack("<4I", a[b"strh"][20:36])
        assert arate / scale == rate and length == pcm.shape[0] and struct.unpack("<I", a[b"strh"][44:48])[0] == 4
        assert struct.unpack("<HHIIHH", a[b"strf"][:16]) == (1, 2, rate, rate * 4, 4, 16)

    video = [(b, s) for cc, b, s in info["chunks"] if cc == b"00dc"]
    audio = [(b, s) for cc, b, s in info["chunks"] if cc == b"01wb"]
    assert len(video) + len(audio) == len(info["chunks"]) and len(video) == n
    assert [buf[b:b + s] for b, s in video] == jpegs
    if with_audio:
        assert b"".join(buf[b:b + s] for b, s in audio) == pcm.astype("<i2").tobytes()           # bit-exact, nothing lost or repeated
        assert all(s == rate // fps * 4 for _, s in audio[:-1])                                   # one video frame's duration each
        order = [cc for cc, _, _ in info["chunks"]]
        assert order[:4] == [b"00dc", b"01wb", b"00dc", b"01wb"]                                  # interleaved
    else:
        assert not audio
    assert len(info["index"]) == len(info["chunks"])
    for (cc, flags, off, ln), (cc2, body, size2) in zip(info["index"], info["chunks"]):
        at = info["movi_fourcc_at"] + off                                                        # idx1 offsets count from the 'movi' fourcc
        assert cc == cc2 and buf[at:at + 4] == cc and struct.unpack("<I", buf[at + 4:at + 8])[0] == ln == size2 and at + 8 == body

    back = inputs.read_frames(str(path))
    assert len(back) == n
    for img, j in zip(back, jpegs):
        assert img.size == (W, H) and img.mode == "RGB"
        assert np.array_equal(np.asarray(img), np.asarray(Image.open(io.BytesIO(j)).convert("RGB")))
    assert len(inputs.read_frames(str(path), 3)) == 3


def test_read_frames_refuses_an_avi_with_another_codec(tmp_path):
    from mmgt_amd import inputs, video_out
    path = tmp_path / "other.avi"
    video_out.write_avi(str(path), [_pil_jpeg(R.smooth_frame(16, 16, 0))], 16, 16, 8)
    buf = path.read_bytes()
    assert buf.count(b"MJPG") == 2
    (tmp_path / "h264.avi").write_bytes(buf.replace(b"MJPG", b"H264"))
    with pytest.raises(RuntimeError, match="needs a video decoder"):
        inputs.read_frames(str(tmp_path / "h264.avi"))
    (tmp_path / "junk.avi").write_bytes(b"not a riff file at all")
    with pytest.raises(RuntimeError, match="needs a video decoder"):
        inputs.read_frames(str(tmp_path / "junk.avi"))


def test_write_avi_refuses_files_past_one_gib(tmp_path, monkeypatch):
    from mmgt_amd import video_out
    monkeypatch.setattr(video_out, "AVI_MAX_BYTES", 4096)
    with pytest.raises(ValueError, match="1 GiB"):
        video_out.write_avi(str(tmp_path / "big.avi"), [_pil_jpeg(R.noise_frame(64, 64, 0), 100)] * 4, 64, 64, 25)
    assert not (tmp_path / "big.avi").exists()
    with pytest.raises(ValueError, match="int16"):
        video_out.write_avi(str(tmp_path / "a.avi"), [_pil_jpeg(R.smooth_frame(16, 16, 0))], 16, 16, 25, audio=(np.zeros(10, np.float32), 8000))
