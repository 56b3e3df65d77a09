"""Uncompressed YUV4MPEG2 (Y4M) files of 8-bit 4:2:0 frames: the reader and the writer behind `convert_y4m` (video.py).  Pure
Python, no GPU.  A file is one header line `YUV4MPEG2 W.. H.. F..:.. [I.] [A..:..] [C..] [X..]...` and then, per frame, a line
`FRAME[ parameters]` followed by the frame's planes (Y, U, V; yuv.py has the layout).  Only what the GPU path converts is taken:
C420jpeg (chroma sited between the luma columns: "center"), C420mpeg2 ("left"), a bare C420 or no C tag (both read as 420jpeg),
progressive frames; everything else is refused with a text that names the tag."""
from __future__ import annotations

from fractions import Fraction

MAGIC = b"YUV4MPEG2"
_SITING_OF = {"420jpeg": "center", "420mpeg2": "left", "420": "center"}
_TAG_OF_SITING = {"center": "420jpeg", "left": "420mpeg2"}
_MAX_LINE = 4096  # header and FRAME lines are short; a longer one is not a Y4M file


def _frame_bytes(w: int, h: int) -> int:
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


def _pair(tag: str, text: str) -> list:
    parts = text.split(":")
    if len(parts) != 2 or not all(p.isdigit() for p in parts):
        raise ValueError(f"Y4M tag {tag}{text}: expected {tag}<int>:<int>")
    return parts


def _ratio(tag: str, text: str) -> Fraction:
    parts = _pair(tag, text)
    if int(parts[1]) == 0:
        raise ValueError(f"Y4M tag {tag}{text}: zero denominator")
    return Fraction(int(parts[0]), int(parts[1]))


def parse_header(line: bytes) -> dict:
    """The fields of a header line (without its newline): width, height, fps (a Fraction), interlace ("p" or "?"; None when the
    tag is absent), aspect (the text after A, or None), colorspace (the text after C, or None), siting, range ("limited" |
    "full"), x_tags (the X tags' texts in order) and tags (every tag as written).  ValueError names the tag that is refused."""
    try:
        words = line.decode("ascii").split(" ")
    except UnicodeDecodeError:
        raise ValueError("not a YUV4MPEG2 header: it is not ASCII") from None
    if words[0] != MAGIC.decode():
        raise ValueError("not a YUV4MPEG2 file: the header does not begin with YUV4MPEG2")
    out = {"width": None, "height": None, "fps": None, "interlace": None, "aspect": None, "colorspace": None, "siting": "center",
           "range": "limited", "x_tags": [], "tags": [w for w in words[1:] if w]}
    for word in out["tags"]:
        key, val = word[0], word[1:]
        if key in "WH":
            if not val.isdigit() or int(val) == 0:
                raise ValueError(f"Y4M tag {word}: expected {key}<positive int>")
            out["width" if key == "W" else "height"] = int(val)
        elif key == "F":
            out["fps"] = _ratio("F", val)
            if out["fps"] <= 0:
                raise ValueError(f"Y4M tag {word}: the frame rate must be positive")
        elif key == "I":
            if val not in ("p", "?"):
                raise ValueError(f"Y4M tag {word}: interlaced video is not supported (only Ip and I?)")
            out["interlace"] = val
        elif key == "A":
            _pair("A", val)  # (A0:0 says "unknown")
            out["aspect"] = val
        elif key == "C":
            if val not in _SITING_OF:
                raise ValueError(f"Y4M tag {word}: only 8-bit 4:2:0 is supported (C420jpeg, C420mpeg2, C420)")
            out["colorspace"], out["siting"] = val, _SITING_OF[val]
        elif key == "X":
            out["x_tags"].append(val)
            if val.startswith("COLORRANGE="):
                rng = val.split("=", 1)[1]
                if rng not in ("FULL", "LIMITED"):
                    raise ValueError(f"Y4M tag {word}: expected XCOLORRANGE=FULL or XCOLORRANGE=LIMITED")
                out["range"] = rng.lower()
        # (any other tag is kept in `tags` and not interpreted)
    for key, name in (("W", "width"), ("H", "height"), ("F", "fps")):
        if out[name] is None:
            raise ValueError(f"Y4M header: the {key} tag is missing")
    return out


def _read_line(fh) -> bytes:
    line = fh.readline(_MAX_LINE)
    if line and not line.endswith(b"\n"):
        raise ValueError("Y4M: a header or FRAME line without its newline" if len(line) < _MAX_LINE else "Y4M: a line longer than 4096 bytes")
    return line


class Y4MReader:
    """`for frame in Y4MReader(path)`: the I420 frames as bytes.  width, height, fps (Fraction), siting ("center" | "left"), range
    ("limited" | "full"), interlace, aspect, colorspace, x_tags and tags come from the header.  ValueError for a header that is
    refused and for a truncated frame."""

    def __init__(self, path):
        self.path = path
        self._fh = open(path, "rb")
        try:
            line = _read_line(self._fh)
            if not line:
                raise ValueError("not a YUV4MPEG2 file: it is empty")
            hdr = parse_header(line[:-1])
        except Exception:
            self._fh.close()
            raise
        self.width, self.height, self.fps = hdr["width"], hdr["height"], hdr["fps"]
        self.interlace, self.aspect, self.colorspace = hdr["interlace"], hdr["aspect"], hdr["colorspace"]
        self.siting, self.range, self.x_tags, self.tags = hdr["siting"], hdr["range"], hdr["x_tags"], hdr["tags"]
        self.frame_bytes = _frame_bytes(self.width, self.height)
        self.frames_read = 0

    def read_frame(self):
        """The next frame, or None at the end of the file."""
        line = _read_line(self._fh)
        if not line:
            return None
        if line != b"FRAME\n" and not line.startswith(b"FRAME "):
            raise ValueError(f"Y4M frame {self.frames_read}: expected a FRAME line, got {line[:16]!r}")
        data = self._fh.read(self.frame_bytes)
        if len(data) != self.frame_bytes:
            raise ValueError(f"Y4M frame {self.frames_read} is truncated: {len(data)} of {self.frame_bytes} bytes")
        self.frames_read += 1
        return data

    def read_frames(self, n: int) -> list:
        """Up to `n` frames (fewer at the end of the file)."""
        out = []
        while len(out) < n:
            f = self.read_frame()
            if f is None:
                break
            out.append(f)
        return out

    def __iter__(self):
        while True:
            f = self.read_frame()
            if f is None:
                return
            yield f

    def close(self):
        self._fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4MWriter:
    """Writes the header on construction, then a `FRAME` line and the bytes per `write(frame)`.  fps: a Fraction or an int; siting
    "center" | "left"; range None (no tag) | "limited" | "full"; interlace None (no tag) | "p" | "?"; aspect None or "N:D";
    colorspace "": the C tag of `siting`; a text (a bare "420"): that spelling, which must say the same siting; None: no C tag
    (readers then assume 420jpeg, so only with siting "center").  x_tags: the X tags' texts to write instead of the one `range`
    gives."""

    def __init__(self, path, width: int, height: int, fps, siting: str = "center", range=None, aspect=None, interlace=None,
                 colorspace="", x_tags=None):
        if int(width) <= 0 or int(height) <= 0:
            raise ValueError("Y4MWriter: width and height must be positive")
        fps = Fraction(fps)
        if fps <= 0:
            raise ValueError("Y4MWriter: the frame rate must be positive")
        if siting not in _TAG_OF_SITING:
            raise ValueError(f"Y4MWriter: siting must be 'center' or 'left', got {siting!r}")
        if range not in (None, "limited", "full"):
            raise ValueError(f"Y4MWriter: range must be None, 'limited' or 'full', got {range!r}")
        if interlace not in (None, "p", "?"):
            raise ValueError(f"Y4MWriter: interlace must be None, 'p' or '?', got {interlace!r}")
        if (colorspace is None and siting != "center") or (colorspace and _SITING_OF.get(colorspace) != siting):
            raise ValueError(f"Y4MWriter: colorspace {colorspace!r} does not say siting {siting!r}")
        self.width, self.height, self.fps = int(width), int(height), fps
        self.frame_bytes = _frame_bytes(self.width, self.height)
        words = [MAGIC.decode(), f"W{self.width}", f"H{self.height}", f"F{fps.numerator}:{fps.denominator}"]
        if interlace is not None:
            words.append("I" + interlace)
        if aspect is not None:
            _pair("A", aspect)
            words.append("A" + aspect)
        if colorspace is not None:  # None: the input had no C tag, and none is written
            words.append("C" + (colorspace or _TAG_OF_SITING[siting]))
        tags = list(x_tags) if x_tags is not None else ([] if range is None else ["COLORRANGE=" + range.upper()])
        words += ["X" + t for t in tags]
        self.frames_written = 0
        self._fh = open(path, "wb")
        self._fh.write(" ".join(words).encode("ascii") + b"\n")

    def write(self, frame) -> None:
        mv = memoryview(frame).cast("B")
        if len(mv) != self.frame_bytes:
            raise ValueError(f"Y4MWriter: a {self.width}x{self.height} frame holds {self.frame_bytes} bytes, got {len(mv)}")
        self._fh.write(b"FRAME\n")
        self._fh.write(mv)
        self.frames_written += 1

    def close(self):
        self._fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
