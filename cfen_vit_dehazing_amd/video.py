"""Dehaze a YUV4MPEG2 (.y4m) stream: reader, writer and the loop of dehaze_video.py.

A y4m stream is one text line (`YUV4MPEG2 W.. H.. F.. I.. A.. C.. X..`) and then, per frame, a `FRAME` line and the planes Y, Cb, Cr as raw
bytes -- what `ffmpeg -f yuv4mpegpipe`, x264, aomenc and vmaf read and write.  The frame bytes go to the device as they are; the colour
conversion both ways runs there (ops.yuv_to_rgb_u8 / ops.rgb_to_yuv_u8, include/cfen_yuv.h) next to the forward.  A stream of 9 to 16 bits per
sample (--video_depth auto) takes the same loop on floats: ops.yuv16_to_rgb_f32 / ops.rgb_f32_to_yuv16 (include/cfen_yuv16.h), no bytes on the way.

Threads: one reader fills pinned host buffers, one writer drains them; the main thread issues, per batch and on ONE stream, the copy in, the
conversion, the forward, the conversion back and the copy out.  The ring holds --video_buffers slots; a slot goes reader -> main -> writer ->
reader.  Everything on the device happens in frame order on that stream, so the output does not depend on timing or on the number of slots.

--eval_gt CLEAR.y4m scores the payload that leaves against a ground-truth stream, plane by plane (ops.plane_metrics, include/cfen_planes.h;
gtscore.py): the main thread reads the ground-truth frames of a batch into the slot's third pinned buffer after the copy out is issued."""
import os
import queue
import sys
import threading
import time

from . import yuv

MAX_HEADER = 8192
ACCEPTED_C = ("420jpeg", "420mpeg2", "422", "444", "mono")
# The deep C tags mjpegtools / ffmpeg define, read with max_depth = 16: {tag value: (chroma, depth)}.  C420pN is read as 4:2:0 CO-SITED (the taps of
# 420mpeg2): chroma on the even columns, between the rows -- the siting of H.264 / HEVC / AV1 output, which is where deep footage comes from (the
# tag itself does not say).  There is no Cmono14.
DEEP_C = dict([("%sp%d" % (c, d), ({"420": "420mpeg2"}.get(c, c), d)) for d in yuv.DEPTHS for c in ("420", "422", "444")] +
              [("mono%d" % d, ("mono", d)) for d in yuv.DEPTHS if d != 14])


class Y4MError(ValueError):
    pass


def _open(target, mode):
    """(binary file object, do we close it): a path, '-' for stdin / stdout, or an open binary file object"""
    if hasattr(target, "read") or hasattr(target, "write"):
        return target, False
    if target == "-":
        return (sys.stdin.buffer if mode == "rb" else sys.stdout.buffer), False
    return open(target, mode), True


def parse_header(line, max_depth=8):
    """the fields of a `YUV4MPEG2 ...` line (bytes, with or without its newline) as a dict: width, height, chroma (one of ACCEPTED_C), depth (8, or
    that of a DEEP_C tag when max_depth allows it), ctag (the C tag as written, or None), color_range ('full' | 'limited' | None), tags (every token
    after the magic).  Y4MError names the tag this project does not read."""
    text = line.rstrip(b"\n").decode("ascii", "replace")
    tokens = text.split(" ")
    if tokens[0] != "YUV4MPEG2":
        raise Y4MError("not a YUV4MPEG2 stream: the first line starts with %r" % text[:16])
    tags = [t for t in tokens[1:] if t]
    info = {"width": None, "height": None, "chroma": "420jpeg", "depth": 8, "ctag": None, "color_range": None, "tags": tags}
    for t in tags:
        key, value = t[0], t[1:]
        if key in "WH":
            if not value.isdigit() or not 1 <= int(value) <= yuv.MAX_EDGE:
                raise Y4MError("y4m header: bad size tag %r (1 .. %d)" % (t, yuv.MAX_EDGE))
            info["width" if key == "W" else "height"] = int(value)
        elif key == "I":
            if value not in ("p", "?"):
                raise Y4MError("y4m header: interlaced stream (tag %r): only progressive frames (Ip) are dehazed" % t)
        elif key == "C":
            info["ctag"] = t
            if value == "420":
                value = "420jpeg"                      # mjpegtools: a plain 420 is 420jpeg
            if value in DEEP_C and DEEP_C[value][1] <= max_depth:
                info["chroma"], info["depth"] = DEEP_C[value]
                continue
            if value not in ACCEPTED_C:
                why = "high bit depth" if "p1" in value or value.endswith("p9") else ("PAL-DV chroma siting" if value == "420paldv" else "unknown chroma format")
                deep = "" if max_depth <= 8 else " and C420pN, C422pN, C444pN, CmonoN for N in %s" % (tuple(d for d in yuv.DEPTHS if d <= max_depth),)
                raise Y4MError("y4m header: tag %r (%s) is not supported: 8-bit %s only%s" % (t, why, ", ".join("C" + c for c in ACCEPTED_C), deep))
            info["chroma"] = value
        elif t.startswith("XCOLORRANGE="):
            r = t.split("=", 1)[1].upper()
            if r not in ("FULL", "LIMITED"):
                raise Y4MError("y4m header: tag %r: XCOLORRANGE is FULL or LIMITED" % t)
            info["color_range"] = r.lower()
    if info["width"] is None or info["height"] is None:
        raise Y4MError("y4m header: no %s tag in %r" % ("W" if info["width"] is None else "H", text))
    return info


def _check_frame_line(line, index):
    """`line`: what readline gave where frame `index` starts (not empty)"""
    if line == b"FRAME\n" or (line.startswith(b"FRAME ") and line.endswith(b"\n")):
        return
    if not line.endswith(b"\n") and (b"FRAME\n".startswith(line) or line.startswith(b"FRAME ")) and len(line) < MAX_HEADER:
        raise Y4MError("y4m frame %d is cut short: the stream ends inside its FRAME line" % index)
    raise Y4MError("y4m frame %d: expected a FRAME line, got %r" % (index, line[:16]))


class Y4MReader:
    """frames of a y4m stream, one at a time.  source: a path, '-' (stdin, binary) or a binary file object.  Reads that come back short (a pipe)
    are continued.  `header` is the first line byte for byte, with its newline.  max_depth: 8 refuses every deep stream, 16 reads the DEEP_C tags;
    `depth` is then the bits per sample and `frame_bytes` counts two bytes per sample."""

    def __init__(self, source, max_depth=8):
        self._f, self._own = _open(source, "rb")
        line = self._f.readline(MAX_HEADER)
        if not line.endswith(b"\n"):
            raise Y4MError("y4m header: no end of line within %d bytes" % MAX_HEADER if len(line) >= MAX_HEADER else "y4m header: the stream ends inside it")
        self.header = line
        info = parse_header(line, max_depth)
        self.width, self.height, self.chroma, self.color_range, self.tags = (info[k] for k in ("width", "height", "chroma", "color_range", "tags"))
        self.depth, self.ctag = info["depth"], info["ctag"]
        self.frame_bytes = yuv.frame_bytes(self.height, self.width, self.chroma, self.depth)
        self.frames_read = 0

    def _fill(self, view):
        """read len(view) bytes; returns how many arrived before the end of the stream"""
        got, n = 0, len(view)
        while got < n:
            k = self._f.readinto(view[got:])
            if not k:
                break
            got += k
        return got

    def read_frame_into(self, buf):
        """the next frame's payload into `buf` (a writable buffer of frame_bytes bytes); False at the end of the stream.  Y4MError naming the
        frame index when the stream ends inside a frame or a FRAME line is missing."""
        line = self._f.readline(MAX_HEADER)
        if not line:
            return False
        _check_frame_line(line, self.frames_read)
        view = memoryview(buf).cast("B")
        if len(view) != self.frame_bytes:
            raise ValueError("read_frame_into needs a buffer of %d bytes, got %d" % (self.frame_bytes, len(view)))
        got = self._fill(view)
        if got != self.frame_bytes:
            raise Y4MError("y4m frame %d is cut short: %d of %d bytes" % (self.frames_read, got, self.frame_bytes))
        self.frames_read += 1
        return True

    def read_frame(self):
        buf = bytearray(self.frame_bytes)
        return bytes(buf) if self.read_frame_into(buf) else None

    def check_whole_file(self):
        """for a seekable source: walk every FRAME line without reading the payloads and return the number of frames, so that a stream cut short
        is refused before any work is done; None for a pipe (there the cut shows when it is reached).  The position is restored."""
        try:
            if not self._f.seekable():
                return None
            start = self._f.tell()
        except (OSError, ValueError, AttributeError):
            return None
        end = self._f.seek(0, os.SEEK_END)
        self._f.seek(start)
        n, pos = 0, start
        try:
            while pos < end:
                line = self._f.readline(MAX_HEADER)
                _check_frame_line(line, n)
                pos += len(line) + self.frame_bytes
                if pos > end:
                    raise Y4MError("y4m frame %d is cut short: %d of %d bytes" % (n, self.frame_bytes - (pos - end), self.frame_bytes))
                self._f.seek(pos)
                n += 1
        finally:
            self._f.seek(start)
        return n

    def close(self):
        if self._own:
            self._f.close()


class Y4MWriter:
    """writes `header` (the input's first line, byte for byte) when the first frame arrives or at close(), then `FRAME\\n` + payload per frame"""

    def __init__(self, target, header):
        if not header.endswith(b"\n"):
            raise ValueError("a y4m header ends with a newline")
        self._target, self._header = target, header
        self._f, self._own = None, False
        self.frames_written = 0

    def _start(self):
        if self._f is None:
            self._f, self._own = _open(self._target, "wb")
            self._f.write(self._header)

    def write_frame(self, payload):
        self._start()
        self._f.write(b"FRAME\n")
        self._f.write(payload)
        self.frames_written += 1

    def close(self):
        self._start()
        self._f.flush()
        if self._own:
            self._f.close()


def pick_matrix(choice, height):
    return ("bt709" if height >= 720 else "bt601") if choice == "auto" else choice


def pick_range(choice, color_range):
    return (color_range or "limited") if choice == "auto" else choice


class Slot:
    """one slot of the ring: `rows_in` and `rows_out` are writable (batch, frame_bytes) uint8 arrays (pinned host memory in run()); the reader sets
    `n` (frames held) and `first` (index of the first one), process() may hang anything else on `extra`"""
    __slots__ = ("rows_in", "rows_out", "n", "first", "done", "extra")

    def __init__(self, rows_in, rows_out, extra=None):
        self.rows_in, self.rows_out, self.extra = rows_in, rows_out, extra
        self.n = self.first = 0
        self.done = None


def pump(reader, writer, batch, slots, process, seconds=None):
    """Move every frame of `reader` through `process` into `writer`, `batch` frames at a time, and return the number of frames.

    One reader thread fills slots, the calling thread hands each filled slot to process(slot) -- which arranges for slot.rows_out[:slot.n] to hold
    the output and returns None or an object whose synchronize() waits for that -- and one writer thread waits and writes.  A slot goes
    reader -> caller -> writer -> reader, so at most len(slots) batches are in the ring and the output is in frame order whatever the timing.
    Failures end the run, never hang it:
      the writer's (a closed pipe, a full disk): the writer keeps handing slots back so that nobody blocks on the ring, wakes the caller, and its
        exception is raised as soon as the caller has returned from the process() it is in;
      the reader's (a stream cut short): every whole frame read before it -- the batches already queued and the part of the batch it happened
        in -- is still processed and written, then its exception is raised;
      process()'s own: raised once the writer has written what was already handed over."""
    free, filled, towrite = queue.Queue(), queue.Queue(), queue.Queue()
    for s in slots:
        free.put(s)
    read_failure, write_failure = [], []
    seconds = seconds if seconds is not None else {}
    seconds.setdefault("wait_for_frames", 0.0)
    seconds.setdefault("issue", 0.0)

    def read_loop():
        index = 0
        while True:
            s = free.get()
            if s is None:
                return
            n = 0
            try:
                while n < batch and reader.read_frame_into(s.rows_in[n]):
                    n += 1
            except BaseException as e:
                read_failure.append(e)
            s.n, s.first = n, index
            index += n
            if n:
                filled.put(s)
            if n < batch or read_failure:
                filled.put(None)
                return

    def write_loop():
        while True:
            s = towrite.get()
            if s is None:
                return
            if not write_failure:
                try:
                    if s.done is not None:
                        s.done.synchronize()
                    for k in range(s.n):
                        writer.write_frame(s.rows_out[k])
                except BaseException as e:
                    write_failure.append(e)
                    filled.put(None)          # wakes the caller if it is waiting for frames
            free.put(s)                       # also after a failure: the ring keeps turning until the caller has seen it

    threads = [threading.Thread(target=read_loop, name="y4m-reader", daemon=True), threading.Thread(target=write_loop, name="y4m-writer", daemon=True)]
    for t in threads:
        t.start()
    frames = 0
    try:
        while True:
            t0 = time.perf_counter()
            s = filled.get()
            seconds["wait_for_frames"] += time.perf_counter() - t0
            if s is None or write_failure:
                break
            t0 = time.perf_counter()
            s.done = process(s)
            towrite.put(s)
            frames += s.n
            seconds["issue"] += time.perf_counter() - t0
    finally:
        towrite.put(None)
        free.put(None)
        threads[1].join()
    if write_failure:
        raise write_failure[0]
    writer.close()
    if read_failure:
        raise read_failure[0]
    return frames


DEEP_REFUSED = ("fit", "temporal", "eval_noref", "eval_flicker")      # uint8 machinery: open for deep streams


def refuse_deep_flags(opt, ctag):
    """a stream of more than 8 bits per sample takes the float route, which has no --fit, --temporal, --eval_noref or --eval_flicker yet: Y4MError
    naming the stream's tag and the flag"""
    asked = ["--" + f for f in DEEP_REFUSED if getattr(opt, f, False)]
    if asked:
        raise Y4MError("the stream is %s (more than 8 bits per sample) and %s %s given: %s work on uint8 frames only and the deep route has none "
                       "of them yet; run without, or convert the stream to 8 bits" % (ctag, ", ".join(asked), "is" if len(asked) == 1 else "are",
                                                                                      ", ".join("--" + f for f in DEEP_REFUSED)))


def peek_deep_tag(path):
    """the C tag of the y4m file at `path` if it is one of DEEP_C, else None (also for anything that is not a readable y4m file: run() says why)"""
    try:
        with open(path, "rb") as f:
            info = parse_header(f.readline(MAX_HEADER), max_depth=16)
    except (OSError, Y4MError):
        return None
    return info["ctag"] if info["depth"] > 8 else None


def peek_header(path, max_depth=8):
    """parse_header of the first line of the y4m file at `path`; OSError if it cannot be read, Y4MError if it is not a stream this project reads"""
    with open(path, "rb") as f:
        return parse_header(f.readline(MAX_HEADER), max_depth)


def _interlacing(info):
    return next((t[1:] for t in info["tags"] if t[0] == "I"), "?")


def check_gt_header(src, gt, gt_name="the ground truth"):
    """--eval_gt: the ground truth's header against the input's (two parse_header dicts): the planes are compared sample by sample, so the size,
    the C tag (and with it the depth) and the interlacing must be equal.  Y4MError naming both values"""
    def ctag(info):
        return info["ctag"] or "C420jpeg (no C tag)"
    same_format = (src["chroma"], src["depth"]) == (gt["chroma"], gt["depth"])          # C420 and no C tag at all are C420jpeg too
    for what, a, b, equal in (("width", src["width"], gt["width"], src["width"] == gt["width"]),
                              ("height", src["height"], gt["height"], src["height"] == gt["height"]),
                              ("C tag", ctag(src), ctag(gt), same_format),
                              ("interlacing", "I" + _interlacing(src), "I" + _interlacing(gt), _interlacing(src) == _interlacing(gt))):
        if not equal:
            raise Y4MError("--eval_gt %s: its %s is %s but the input's is %s: a ground truth is compared sample by sample and needs the input's "
                           "size, C tag and interlacing" % (gt_name, what, b, a))


class UnsafeHalfFrames(Y4MError):
    """--precision half: a guard check failed after fp16 frames had already left in the stream"""


def run(opt, log=print):
    """the loop of dehaze_video.py.  opt: VideoOptions().parse().  Returns the number of frames.  Everything printed goes through `log` (stderr when
    the video leaves on stdout)."""
    import torch
    from . import metrics, ops
    from .models import create_model

    deep_allowed = getattr(opt, "video_depth", "8") == "auto"
    reader = Y4MReader(opt.video_in, max_depth=16 if deep_allowed else 8)
    H, W, chroma, depth = reader.height, reader.width, reader.chroma, reader.depth
    deep = depth > 8
    if deep:
        refuse_deep_flags(opt, reader.ctag)   # a pipe: as soon as the header is read, before the checkpoint is loaded and before any output
    gt_reader = None
    if getattr(opt, "eval_gt", None):
        # as the deep refusal above: for a piped input this is the first moment the two headers can be compared
        gt_reader = Y4MReader(opt.eval_gt, max_depth=16 if deep_allowed else 8)
        check_gt_header(parse_header(reader.header, 16 if deep_allowed else 8), parse_header(gt_reader.header, 16 if deep_allowed else 8), opt.eval_gt)
    matrix = pick_matrix(opt.video_matrix, H)
    full = pick_range(opt.video_range, reader.color_range) == "full"
    log("video: %d x %d C%s%s, matrix %s (%s), range %s (%s)" % (W, H, chroma, ", %d bits per sample (%s)" % (depth, "float route" if deep else "uint8 route")
                                                                 if deep_allowed else "", matrix,
                                                                 "auto: H >= 720 is bt709" if opt.video_matrix == "auto" else "given",
                                                                 "full" if full else "limited",
                                                                 ("auto: XCOLORRANGE" if reader.color_range else "auto: no XCOLORRANGE tag") if opt.video_range == "auto" else "given"))
    from .config import VARIANTS, FULL_RES_VARIANTS
    T = opt.loadSize if VARIANTS.get(opt.model_G, "v3") in FULL_RES_VARIANTS else 2 * opt.loadSize      # the generator's image edge (as in test.py)
    route = "plain" if (H, W) == (T, T) else ("fit" if opt.fit else ("tile" if opt.tile else None))
    if route is None:
        raise Y4MError("the frames are %d x %d but the generator takes %d x %d: give %s--tile (overlapping tiles)"
                       % (W, H, T, T, "" if deep else "--fit (one resampled forward per frame) or "))
    n_known = reader.check_whole_file()       # a file cut short is refused here, before any forward
    if gt_reader is not None:
        gt_known = gt_reader.check_whole_file()
        if n_known is not None and gt_known is not None and gt_known < n_known:
            raise Y4MError("--eval_gt %s holds %d frames but the input holds %d: frame %d has no ground truth" % (opt.eval_gt, gt_known, n_known, gt_known))
    model = create_model(opt)
    model.setup(opt)
    model.set_noref_scoring(False)            # the frames are scored here (all three routes), not in model.test()
    net = model.netG
    if net.cfg.image_size != T:
        raise RuntimeError("the generator's image size is %d, expected %d" % (net.cfg.image_size, T))
    if route == "plain":
        model.use_native_size_route()         # frames of the generator's own size: the plain --u8_input route whatever was asked for other sizes
    if deep:
        model.use_float_outputs()             # the deep route quantises the generator's floats itself (ops.rgb_f32_to_yuv16)
    nb, B = reader.frame_bytes, opt.batchSize
    dev = model.device
    stream = torch.cuda.current_stream()
    writer = Y4MWriter(opt.video_out, reader.header)
    slots = []
    for _ in range(opt.video_buffers):
        pins = (torch.empty(B, nb, dtype=torch.uint8).pin_memory(), torch.empty(B, nb, dtype=torch.uint8).pin_memory())
        if gt_reader is not None:
            pins += (torch.empty(B, nb, dtype=torch.uint8).pin_memory(),)          # the ground truth of the slot's frames
        slots.append(Slot(pins[0].numpy(), pins[1].numpy(), extra=pins))
    d_in = torch.empty(B, nb, dtype=torch.uint8, device=dev)
    d_out = torch.empty(B, nb, dtype=torch.uint8, device=dev)
    rgb = torch.empty((B, 3, H, W) if deep else (B, H, W, 3), dtype=torch.float32 if deep else torch.uint8, device=dev)
    noref_rows = []
    seconds = {"wait_for_frames": 0.0, "issue": 0.0, "noref": 0.0}
    actnorm = {"ready": False}                # asked of the device until it is true, then remembered (the layers never go back)
    stabiliser = None
    if getattr(opt, "temporal", False):
        from . import temporal
        mc = getattr(opt, "temporal_mc", None) or 0
        subpel = (getattr(opt, "temporal_mc_subpel", None) or 1) if mc else 1
        stabiliser = temporal.Stabiliser(opt.temporal_radius, opt.temporal_eps, opt.temporal_strength, opt.temporal_motion, opt.temporal_down,
                                         **(dict(mc_range=mc, mc_block=opt.temporal_mc_block, mc_bias=opt.temporal_mc_bias) if mc else {}),
                                         **(dict(mc_subpel=subpel) if subpel > 1 else {}))
        S, h, w = temporal.working_size(H, W, stabiliser.down)
        log("video: temporal stabilisation at %d x %d (1/%d), radius %d, eps %g, strength %g, motion %g levels"
            % (w, h, S, stabiliser.radius, stabiliser.eps, stabiliser.strength, stabiliser.motion))
        if mc:
            log("video: motion compensation within +-%d pixels, blocks of %d x %d, bias %d / 16 levels per pixel"
                % (stabiliser.mc_range, stabiliser.mc_block, stabiliser.mc_block, stabiliser.mc_bias))
        if subpel > 1:
            log("video: vectors refined to 1/%d pixel" % stabiliser.mc_subpel)

    scorer, flicker_rows = None, []
    if getattr(opt, "eval_flicker", False):
        from . import flicker
        scorer = flicker.Scorer(opt.flicker_range, opt.flicker_block, opt.flicker_bias, opt.flicker_tol, opt.flicker_down)
        seconds["flicker"] = 0.0
        S, h, w = scorer.working_size(H, W)
        log("video: flicker along the motion at %d x %d (1/%d), search within +-%d pixels, blocks of %d x %d, bias %d / 16, tolerance %d levels"
            % (w, h, S, scorer.range, scorer.block, scorer.block, scorer.bias, scorer.tol))

    gt_scorer, gt_rows, d_gt = None, [], None
    if gt_reader is not None:
        from . import gtscore
        gt_scorer = gtscore.Scorer(H, W, chroma, depth)
        d_gt = torch.empty(B, nb, dtype=torch.uint8, device=dev)
        seconds["gt"] = 0.0
        log("video: scoring against %s, per plane on the %d-bit samples that leave" % (opt.eval_gt, depth))

    def score_gt(s):
        """--eval_gt: the slot's ground-truth frames go through the slot's pinned buffer to the device and are compared with the payload in d_out,
        the very bytes that leave.  The call waits for its own results, so the pinned buffer is free again when the slot comes back."""
        t1 = time.perf_counter()
        pin_gt = s.extra[2]
        rows_gt = pin_gt.numpy()
        for k in range(s.n):
            if not gt_reader.read_frame_into(rows_gt[k]):
                raise Y4MError("--eval_gt %s ends before frame %d of the input: every frame needs its ground truth" % (opt.eval_gt, s.first + k))
        d_gt[:s.n].copy_(pin_gt[:s.n], non_blocking=True)
        for k, row in enumerate(gt_scorer.step(d_out[:s.n], d_gt[:s.n])):
            gt_rows.append(("frame_%06d" % (s.first + k), row))
        seconds["gt"] += time.perf_counter() - t1

    def through_model(x, first):
        """the model's own batch route, the one test.py takes (the half guard included where test.py applies it)"""
        model.set_input({"B": x, "B_paths": ["frame_%06d" % (first + k) for k in range(x.shape[0])]})
        model.test(opt)
        return model.output_bytes()

    def process_deep(s):
        """the float route of a stream of 9 .. 16 bits per sample: the samples become (n,3,H,W) float32 in [-1, 1] (include/cfen_yuv16.h), the
        generator's float outputs are rounded to samples of the same depth; nothing on the way is a byte"""
        n = s.n
        pin_in, pin_out = s.extra[:2]
        d_in[:n].copy_(pin_in[:n], non_blocking=True)
        x = ops.yuv16_to_rgb_f32(d_in[:n], H, W, chroma, depth, matrix, full, out=rgb[:n])

        def model_floats(xs, first):
            model.set_input({"B": xs, "B_paths": ["frame_%06d" % (first + k) for k in range(xs.shape[0])]})
            model.test(opt)
            return model.output_floats()
        if route != "tile":
            y = model_floats(x, s.first)
        else:
            parts, lo = [], 0
            if not actnorm["ready"]:
                actnorm["ready"] = model.actnorm_ready()
            if not actnorm["ready"]:
                parts.append(model_floats(x[:1], s.first))       # as the uint8 route: the first frame alone initialises the ActNorm layers
                actnorm["ready"] = model.actnorm_ready()
                lo = 1
            if lo < n:
                with torch.no_grad():
                    outs = net.forward_tiled_many([x[k] for k in range(lo, n)], overlap=opt.tile_overlap, tile_batch=opt.tile_batch, output_u8=False,
                                                  self_ensemble=bool(getattr(opt, "self_ensemble", False)))
                parts.append(torch.stack([o[2].float() for o in outs]))
            y = parts[0] if len(parts) == 1 else torch.cat(parts)
        ops.rgb_f32_to_yuv16(y.contiguous(), chroma, depth, matrix, full, out=d_out[:n])
        pin_out[:n].copy_(d_out[:n], non_blocking=True)
        done = torch.cuda.Event()
        done.record(stream)
        if gt_scorer is not None:
            score_gt(s)                       # after the copy out is on its way: the writer does not wait for the scores
        return done

    def process(s):
        n = s.n
        pin_in, pin_out = s.extra[:2]
        d_in[:n].copy_(pin_in[:n], non_blocking=True)
        x = ops.yuv_to_rgb_u8(d_in[:n], H, W, chroma, matrix, full, out=rgb[:n])
        if route != "tile":
            y = through_model(x, s.first)
        else:
            parts, lo = [], 0
            if not actnorm["ready"]:
                actnorm["ready"] = model.actnorm_ready()
            if not actnorm["ready"]:
                # the very first frame of a checkpoint whose ActNorm layers are uninitialised runs alone through the model's route, which
                # initialises them from it as test.py --tile does with its first image
                parts.append(through_model(x[:1], s.first))
                actnorm["ready"] = model.actnorm_ready()
                lo = 1
            if lo < n:
                with torch.no_grad():
                    outs = net.forward_tiled_many([x[k] for k in range(lo, n)], overlap=opt.tile_overlap, tile_batch=opt.tile_batch, output_u8=True,
                                                  self_ensemble=bool(getattr(opt, "self_ensemble", False)))
                parts.append(torch.stack([o[2] for o in outs]))
            y = parts[0] if len(parts) == 1 else torch.cat(parts)
        y = y.contiguous()
        y_net = y
        if stabiliser is not None:
            y = stabiliser.step(x, y)         # all three routes; --eval_noref scores, and the stream carries, the stabilised bytes
        if scorer is not None:
            t1 = time.perf_counter()
            rows = scorer.step(x, y_net, y)   # the network's bytes and the bytes that leave, over the same pixels
            for j, row in enumerate(rows):    # every frame of the batch but the very first of the stream
                flicker_rows.append(("frame_%06d" % (s.first + n - len(rows) + j), row))
            seconds["flicker"] += time.perf_counter() - t1
        if opt.eval_noref:
            t1 = time.perf_counter()
            for k, row in enumerate(metrics.noref(x, y, opt.noref_radius)):
                noref_rows.append(("frame_%06d" % (s.first + k),) + tuple(row))
            seconds["noref"] += time.perf_counter() - t1
        ops.rgb_to_yuv_u8(y, chroma, matrix, full, out=d_out[:n])
        pin_out[:n].copy_(d_out[:n], non_blocking=True)
        done = torch.cuda.Event()
        done.record(stream)
        if gt_scorer is not None:
            score_gt(s)                       # after the copy out is on its way: the writer does not wait for the scores
        return done

    t_start = time.perf_counter()
    frames = pump(reader, writer, B, slots, process_deep if deep else process, seconds)
    reader.close()
    total = time.perf_counter() - t_start
    if n_known is not None and n_known != frames:
        raise Y4MError("read %d frames of the %d the file holds" % (frames, n_known))
    model.finish_half_guard()
    if opt.eval_noref:
        with open(opt.noref_csv, "w") as f:
            f.write(metrics.format_noref_csv(noref_rows))
        log(metrics.noref_summary_line(noref_rows))
        log("noref: wrote %s" % opt.noref_csv)
    if scorer is not None:
        with open(opt.flicker_csv, "w") as f:
            f.write(flicker.format_csv(flicker_rows))
        log(flicker.summary_line([r for _, r in flicker_rows]))
        log("flicker: wrote %s" % opt.flicker_csv)
    if gt_scorer is not None:
        with open(opt.gt_csv, "w") as f:
            f.write(gtscore.format_csv(gt_rows))
        log(gtscore.summary_line([r for _, r in gt_rows]))
        log("gt: wrote %s" % opt.gt_csv)
        extra = gt_reader.read_frame_into(bytearray(nb))
        gt_reader.close()
        if extra:
            raise Y4MError("--eval_gt %s holds more frames than the %d of the input: the two streams do not belong together" % (opt.eval_gt, frames))
    log("video: route %s, %d frames per batch, %d buffers; main-thread seconds %s" % (route, B, opt.video_buffers, {k: round(v, 3) for k, v in seconds.items()}))
    log("video: %d frames in %.2f s = %.1f frames/s stream to stream" % (frames, total, frames / max(total, 1e-9)))
    if model.redo_paths:
        # test.py runs such images again in fp32 and rewrites their files; a stream has already left.  The run must not look like a success.
        raise UnsafeHalfFrames("a --precision half check failed after %d frames (%s .. %s) had been written from fp16 forwards that are now known "
                               "to be unsafe; a stream cannot be rewritten: the output is not to be used, run again with --precision single"
                               % (len(model.redo_paths), model.redo_paths[0], model.redo_paths[-1]))
    return frames
