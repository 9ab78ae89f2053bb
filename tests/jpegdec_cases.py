"""The JPEG streams the decoder tests share (tests/test_jpegdec.py against PIL on the host, tests/test_jpegdec_gpu.py against tests/jpegdec_ref.py
on the device): name -> bytes, built once per process.  Everything is seeded; PIL only WRITES files here (any libjpeg writes valid ones)."""
import functools
import io

from PIL import Image

from tests import mjpeg_ref as M


def pil_jpeg(frame, **kw):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def strip_dht(data):
    """The file without its DHT segments (the form Motion-JPEG frames are commonly written in).  Only for files coded with the Annex K tables."""
    out, pos = bytearray(data[:2]), 2
    while True:
        m, length = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        if m != 0xC4:
            out += data[pos:pos + 2 + length]
        pos += 2 + length
        if m == 0xDA:
            return bytes(out) + data[pos:]


@functools.lru_cache(maxsize=None)
def streams():
    out = {}
    for (H, W) in ((16, 16), (21, 37), (48, 64), (33, 18)):
        for ss in ("4:2:0", "4:4:4"):
            for q in (50, 90, 100):
                for kind, fn in (("smooth", M.smooth_frame), ("noise", M.noise_frame)):
                    out[f"ref_{H}x{W}_{ss.replace(':', '')}_q{q}_{kind}"] = M.encode(fn(H, W, 7 * H + W + q), q, ss)
    f = M.smooth_frame(37, 53, 11, sigma=12.0)
    out["pil_default"] = pil_jpeg(f)
    out["pil_optimize"] = pil_jpeg(f, optimize=True)
    for ss in (0, 1, 2):
        out[f"pil_subsampling{ss}"] = pil_jpeg(f, subsampling=ss, quality=92)
    out["pil_restart_blocks3"] = pil_jpeg(f, restart_marker_blocks=3)
    out["pil_restart_rows1"] = pil_jpeg(f, restart_marker_rows=1)
    out["pil_grey"] = pil_jpeg(f[..., 1])
    out["pil_default_no_dht"] = strip_dht(out["pil_default"])
    for W in (3, 4):
        g = M.noise_frame(5, W, 40 + W)
        out[f"narrow_420_w{W}"] = pil_jpeg(g, subsampling=2, quality=95)
        out[f"narrow_422_w{W}"] = pil_jpeg(g, subsampling=1, quality=95)
    return out


def names():
    return sorted(streams())
