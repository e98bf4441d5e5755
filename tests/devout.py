"""eu_hip_render (and eu_hip_render_samples / eu_hip_render_rgbe) into the CALLER's device memory: a buffer that
is all fill word before the call, with guards in front of and behind the rows and padding behind every row, so
that what the kernels wrote - and where - can be told from what they left alone. TEST CODE.

envutil_amd.render() renders into the library's own frame buffer with a dense stride and copies the requested rows
to the host: a store beside, above or below the rows lands in the library's slack and is never seen, and a pixel a
kernel skipped still holds what the previous job left there. Here every call starts from the fill word 0x7FA5A5A5, a
signalling NaN no arithmetic yields and no finite image holds (bytes of 0xA5 for the 8- and 16-bit entries).

    Guarded     the buffer: GUARD + lead units | rows of (row units + pad) | GUARD units
    render_dev  one job into a fresh Guarded: (frame, outside_ok, n_touched)
    held        a case's three assertions: (a) the frame is the oracle's bit for bit, (b) no word of it is still
                the fill word, (c) nothing outside the rows was touched

The entries that write several frames in one call (eu_hip_render_views, eu_hip_render_views_multi,
eu_hip_render_layers) and eu_hip_render_rays have an outer stride of their own:

    GuardedFrames   GUARD + lead words | n frames, each rows of (row words + pad) and then gap words | GUARD words
    views_into, layers_into, rays_into   one call through the C ABI, out_on_device = 1, into a GuardedFrames
    held_frames     (a), (b), (c) for every frame of the buffer; untouched: the whole buffer is still fill

Both buffers take device="cpu": the index arithmetic of outside() and frames() is then tested without a GPU
(tests/test_devout_host.py).
"""
import ctypes as C

import numpy as np

import envutil_amd as ea
import jobs
from envutil_amd import api

FILL = 0x7FA5A5A5
FILL_BYTE = 0xA5
GUARD = 4096          # words in front of and behind the rows (bytes x 4 for the 8- and 16-bit entries)

# entry: bytes per unit of its buffer; a unit is what `pad` and `lead` count
_UNITS = {"render": 4, "samples8": 1, "samples16": 2, "rgbe": 4}


class Outside:
    """the outcome of the outside check: true when every guard, lead and padding unit still holds the fill"""

    def __init__(self, count, first=None):
        self.count, self.first = count, first

    def __bool__(self):
        return self.count == 0

    def __str__(self):
        if not self.count:
            return "nothing outside the rows was touched"
        if len(self.first) == 3:
            return f"{self.count} words outside the frames' rows were written, the first at (frame {self.first[0]}, " \
                   f"row {self.first[1]}, column {self.first[2]})"
        return f"{self.count} words (bytes of a byte buffer) outside the rows were written, the first at (row {self.first[0]}, column {self.first[1]}) of the frame"


class Guarded:
    """`rows` rows of `row_units` units (+ `pad`) between two guards, on the device, all fill. words=True: units are
    32-bit words (an int32 tensor: the fill word is positive there, and torch compares int32 on every build);
    words=False: bytes, `unit` of them per unit"""

    def __init__(self, rows, row_units, pad=0, lead=0, words=True, unit=None, guard=GUARD, device="cuda"):
        import torch
        self.words = words
        self.unit = 4 if words else (unit or 1)          # bytes per unit
        per = 1 if words else self.unit                  # tensor elements per unit
        self.fill = FILL if words else FILL_BYTE
        self.rows, self.row_len, self.stride = rows, row_units * per, (row_units + pad) * per
        self.start = (guard * (1 if words else 4)) + lead * per
        self.total = self.start + rows * self.stride + guard * (1 if words else 4)
        self.buf = torch.full((self.total,), self.fill, dtype=torch.int32 if words else torch.uint8, device=device)
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()                     # the fill ran on torch's stream, the job runs on another

    @property
    def stride_bytes(self):
        return self.stride * self.buf.element_size()

    def ptr(self, row=0):
        return self.buf.data_ptr() + (self.start + row * self.stride) * self.buf.element_size()

    def body(self):
        return self.buf[self.start:self.start + self.rows * self.stride].view(self.rows, self.stride)

    def frame(self):
        """the rows without their padding, on the host: uint32 words or bytes, (rows, row length)"""
        a = self.body()[:, :self.row_len].contiguous().cpu().numpy()
        return a.view(np.uint32) if self.words else a

    def outside(self):
        """counted on the device; the position of the first touched unit is looked up only when there is one"""
        end = self.start + self.rows * self.stride
        parts = [(self.buf[:self.start], 0), (self.buf[end:], end)]
        n = sum(int((p != self.fill).sum().item()) for p, _ in parts)
        padding = self.body()[:, self.row_len:]
        n += int((padding != self.fill).sum().item()) if padding.numel() else 0
        if not n:
            return Outside(0)
        first = None
        for p, base in parts[:1] + [(None, None)] + parts[1:]:
            if p is None:
                if padding.numel():
                    hit = (padding != self.fill).nonzero()
                    if hit.numel():
                        first = (int(hit[0, 0]), self.row_len + int(hit[0, 1]))
            else:
                hit = (p != self.fill).nonzero()
                if hit.numel():
                    first = divmod(base + int(hit[0, 0]) - self.start, self.stride)
            if first is not None:
                break
        return Outside(n, first)


class GuardedFrames:
    """`n` frames between two guards, all fill, 32-bit words (an int32 tensor, as Guarded's): a frame is `rows` rows of
    `row_units` words (+ `pad`) followed by `gap` words, so the frame stride is rows * (row_units + pad) + gap - with
    a gap that is no multiple of the row stride the frames' rows do not lie on one grid. The first frame starts `lead`
    words behind the front guard.

    A word outside the rows is named (frame, row, column) by the frame whose first word precedes it - frame 0 for
    the front guard and the lead, which get negative rows: row and column count in row strides from that frame's first
    word, so a padding word has a column >= row_units and a gap or back-guard word a row >= rows."""

    def __init__(self, n, rows, row_units, pad=0, lead=0, gap=0, guard=GUARD, device="cuda"):
        import torch
        assert n >= 1 and rows >= 1 and row_units >= 1 and min(pad, lead, gap, guard) >= 0
        self.n, self.rows, self.row_len, self.stride, self.gap = n, rows, row_units, row_units + pad, gap
        self.fill = FILL
        self.frame_stride = rows * self.stride + gap
        self.start = guard + lead
        self.end = self.start + n * self.frame_stride
        self.total = self.end + guard
        self.buf = torch.full((self.total,), FILL, dtype=torch.int32, device=device)
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()                     # the fill ran on torch's stream, the call runs on another

    @property
    def stride_bytes(self):
        return self.stride * 4

    @property
    def frame_stride_bytes(self):
        return self.frame_stride * 4

    def ptr(self, frame=0, row=0):
        return self.buf.data_ptr() + (self.start + frame * self.frame_stride + row * self.stride) * 4

    def _parts(self):
        """views of the buffer: front guard + lead, back guard, the rows (n, rows, stride), the gaps (n, gap)"""
        body = self.buf[self.start:self.end].view(self.n, self.frame_stride)
        rows = body[:, :self.rows * self.stride].unflatten(1, (self.rows, self.stride))
        return self.buf[:self.start], self.buf[self.end:], rows, body[:, self.rows * self.stride:]

    def frames(self):
        """the rows without their padding, on the host: uint32 words, (n, rows, row_units)"""
        return self._parts()[2][:, :, :self.row_len].contiguous().cpu().numpy().view(np.uint32)

    def where(self, index):
        """(frame, row, column) of the buffer's word `index`, as the class comment names them"""
        j = index - self.start
        f = min(max(j // self.frame_stride, 0), self.n - 1)
        return (f,) + divmod(j - f * self.frame_stride, self.stride)

    def outside(self):
        """counted on the device; the position of the first touched word is looked up only when there is one"""
        head, tail, rows, gaps = self._parts()
        padding = rows[:, :, self.row_len:]
        parts = [p for p in (head, tail, padding, gaps) if p.numel()]
        n = int(sum((p != self.fill).sum() for p in parts))
        if not n:
            return Outside(0)
        found = []
        for p, index in ((head, lambda h: int(h[0])),
                         (tail, lambda h: self.end + int(h[0])),
                         (padding, lambda h: self.start + int(h[0]) * self.frame_stride + int(h[1]) * self.stride + self.row_len + int(h[2])),
                         (gaps, lambda h: self.start + int(h[0]) * self.frame_stride + self.rows * self.stride + int(h[1]))):
            if p.numel():
                hit = (p != self.fill).nonzero()            # in the order of the addresses
                if hit.numel():
                    found.append(index(hit[0]))
        return Outside(n, self.where(min(found)))


def out_channels(args, nch, stage=0):
    """32-bit words per pixel of an eu_hip_render frame: 3 for stages 1-4, 1 for EU_OUT_SRGBA8, else nchannels"""
    return 1 if args.tethered else 3 if stage else nch


def call_into(buf, args, sources, nch, row_begin=0, row_end=None, stage=0, band=None, stream=None, entry="render",
              first_row=0, **entry_kw):
    """one call of the entry point, out_on_device = 1, into `buf` from its row `first_row` on; asynchronous. Returns the
    rows the call covers"""
    if not isinstance(sources, (list, tuple)):
        sources = [sources]
    t = args.target(nch, row_begin, row_end, stage, band)
    arr = (C.c_void_p * len(sources))(*[s.handle for s in sources])
    st = C.c_void_p(stream) if stream else None
    out = C.c_void_p(buf.ptr(first_row))
    L = ea.lib()
    if entry == "render":
        rc = L.eu_hip_render(C.byref(t), arr, len(sources), out, buf.stride_bytes, 1, st)
    elif entry in ("samples8", "samples16"):
        e, keep = api._encode_struct("render_samples", 8 if entry == "samples8" else 16, entry_kw.get("colour_steps"),
                                     entry_kw.get("alpha_steps"), entry_kw.get("maxval"), entry_kw.get("big_endian", False))
        rc = L.eu_hip_render_samples(C.byref(t), arr, len(sources), C.byref(e), out, buf.stride_bytes, 1, st)
    elif entry == "rgbe":
        rc = L.eu_hip_render_rgbe(C.byref(t), arr, len(sources), out, buf.stride_bytes, 1, st)
    else:
        raise ValueError(entry)
    assert rc == 0, L.eu_hip_last_error().decode()
    return t.row_end - t.row_begin


def typed(frame, args, nch, stage=0, entry="render"):
    """Guarded.frame() as the job's type: (rows, width, och) float32, (rows, width) uint32 for a tethered job,
    (rows, width, nch) uint8 / uint16 samples, (rows, width, 4) uint8 quads"""
    rows, w = frame.shape[0], args.out_width
    if entry == "render":
        return frame.reshape(rows, w) if args.tethered else frame.view(np.float32).reshape(rows, w, out_channels(args, nch, stage))
    if entry == "samples16":
        return np.ascontiguousarray(frame).view(np.uint16).reshape(rows, w, nch)
    return frame.reshape(rows, w, nch if entry == "samples8" else 4)


def render_dev(args, sources, nch, row_begin=0, row_end=None, stage=0, band=None, pad=0, lead=0, stream=None,
               entry="render", **entry_kw):
    """The job into a fresh guarded device buffer whose rows are `pad` units longer than the frame's and start `lead`
    units behind the front guard (units: 32-bit words for entry "render", samples for "samples8" / "samples16", quads for
    "rgbe"). Returns (frame, outside_ok, n_touched): the rows without their padding as the job's type; whether guards,
    lead and padding still hold the fill (an Outside: str() names the first touched unit); the units that do not."""
    t = args.target(nch, row_begin, row_end, stage, band)
    rows, w = t.row_end - t.row_begin, args.out_width
    if entry == "render":
        buf = Guarded(rows, w * out_channels(args, nch, stage), pad, lead)
    else:
        # a quad is one unit of four bytes, a sample one unit of one or two
        buf = Guarded(rows, w * (1 if entry == "rgbe" else nch), pad, lead, words=False, unit=_UNITS[entry])
    call_into(buf, args, sources, nch, row_begin, row_end, stage, band, stream, entry, **entry_kw)
    ea.sync()
    outside = buf.outside()
    return typed(buf.frame(), args, nch, stage, entry), outside, outside.count


def _at(index):
    return tuple(int(v) for v in index)


def words_of(a):
    """what is compared: the float frame's bit patterns, words and bytes as they are"""
    return jobs.bits(a) if a.dtype == np.float32 else a


def check(what, frame, outside, ref, probes=None):
    """(a), (b), (c) on a frame already rendered; prints the case's line for the log. (b) is for 32-bit words: among
    bytes 0xA5 is a sample like any other, and an unwritten one shows in (a) wherever the oracle's byte is another"""
    got, want = words_of(frame), words_of(ref)
    unwritten = int((got == FILL).sum()) if got.dtype == np.uint32 else 0
    print(f"{what}: touched outside {outside.count}, frame words still fill {unwritten}, probes {probes or {}}")
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert unwritten == 0, f"{what}: {unwritten} of {got.size} words of the frame were never written, the first at " \
                           f"{_at(np.argwhere(got == FILL)[0])}"
    bad = np.argwhere(got != want)
    assert not bad.size, f"{what}: {len(bad)} of {got.size} differ from the oracle, the first at {_at(bad[0])}: " \
                         f"{frame[tuple(bad[0])]!r} oracle {ref[tuple(bad[0])]!r}"
    assert outside, f"{what}: {outside}"


def held(what, args, osrc, sources, nch, ref=None, encode=None, probes=None, **kw):
    """One case: render_dev(args, sources, nch, **kw) against jobs.oracle_render of the same rows (`ref`: the oracle's
    frame of these rows, where a caller shares it between cases; `encode`: what turns the oracle's float frame into the
    entry's samples or quads). `probes`: a function called right after the job, its result printed - the
    "this path ran" counters. Returns (frame, probes' result)."""
    if ref is None:
        ref = jobs.oracle_render(args, osrc, stage=kw.get("stage", 0), row_begin=kw.get("row_begin", 0),
                                 row_end=kw.get("row_end"), nch=nch)
        if encode is not None:
            ref = encode(ref)
    frame, outside, _ = render_dev(args, sources, nch, **kw)
    seen = probes() if probes else None
    check(what, frame, outside, ref, seen)
    return frame, seen


def rendered(what, args, sources, nch=None, row_begin=0, row_end=None, **kw):
    """envutil_amd.render()'s frame, rendered into a fresh guarded buffer on the device: (b) and (c) are asserted here,
    the frame is the caller's to compare. For the A/B helpers that render one job under several switches: every
    variant starts from the fill word, not from the pixels the variant before it left in the library's frame buffer."""
    srcs = sources if isinstance(sources, (list, tuple)) else [sources]
    nch = nch or srcs[0].fct.nchannels
    frame, outside, _ = render_dev(args, sources, nch, row_begin, row_end, **kw)
    got = words_of(frame)
    unwritten = int((got == FILL).sum())
    print(f"{what}: touched outside {outside.count}, frame words still fill {unwritten}")
    assert unwritten == 0, f"{what}: {unwritten} of {got.size} words of the frame were never written, the first at " \
                           f"{_at(np.argwhere(got == FILL)[0])}"
    assert outside, f"{what}: {outside}"
    return frame


# ---- several frames in one call: eu_hip_render_views(_multi), eu_hip_render_layers, and eu_hip_render_rays --------
def _stream(stream):
    return C.c_void_p(stream) if stream else None


def views_into(buf, args, views, sources, nch, stream=None, first=0):
    """eu_hip_render_views (a Source) or eu_hip_render_views_multi (a list of them), out_on_device = 1, into `buf` from
    its frame `first` on, with buf's row and frame strides; asynchronous"""
    t = args.target(nch)
    arr = api._views_struct(args, views)
    where = (C.c_void_p(buf.ptr(first)), buf.stride_bytes, buf.frame_stride_bytes, 1, _stream(stream))
    L = ea.lib()
    if isinstance(sources, (list, tuple)):
        handles = (C.c_void_p * len(sources))(*[s.handle for s in sources])
        rc = L.eu_hip_render_views_multi(C.byref(t), arr, len(views), handles, len(sources), *where)
    else:
        rc = L.eu_hip_render_views(C.byref(t), arr, len(views), sources.handle, *where)
    assert rc == 0, L.eu_hip_last_error().decode()


def layers_into(buf, args, layers, nch, stream=None, first=0):
    """eu_hip_render_layers, out_on_device = 1, into `buf` from its frame `first` on; asynchronous"""
    t = args.target(nch)
    handles = (C.c_void_p * max(len(layers), 1))(*[s.handle for s in layers])
    L = ea.lib()
    rc = L.eu_hip_render_layers(C.byref(t), handles, len(layers), C.c_void_p(buf.ptr(first)), buf.stride_bytes,
                                buf.frame_stride_bytes, 1, _stream(stream))
    assert rc == 0, L.eu_hip_last_error().decode()


def rays_into(buf, source, rays, nch=None, taps=None, stream=None):
    """eu_hip_render_rays, out_on_device = 1, into frame 0 of `buf`: `rays` as envutil_amd.render_rays takes them
    (numpy: the staged route; a torch tensor on the device, its rows padded or not: asynchronous). Returns what the
    call points into, for the caller to keep until sync()"""
    r, _, keep = api._rays_struct(source, rays, nch, taps)
    assert (r.height, r.width * r.nchannels) == (buf.rows, buf.row_len), (r.height, r.width, r.nchannels)
    L = ea.lib()
    rc = L.eu_hip_render_rays(C.byref(r), source.handle, C.c_void_p(buf.ptr()), buf.stride_bytes, 1, _stream(stream))
    assert rc == 0, L.eu_hip_last_error().decode()
    return keep


def check_frames(what, got, outside, refs):
    """(a), (b), (c) on frames already rendered: `got` is GuardedFrames.frames(), `refs` the oracle's frame of every
    one of them (float32; its shape may split the row's words into pixels and channels). Prints the case's line"""
    n, rows, row_len = got.shape
    want = [words_of(np.asarray(r)).reshape(-1, row_len) for r in refs]
    unwritten = int((got == FILL).sum())
    print(f"{what}: touched outside {outside.count}, frame words still fill {unwritten}")
    assert len(want) == n and all(w.shape == (rows, row_len) for w in want), (what, got.shape, [w.shape for w in want])
    for k in range(n):
        miss = np.argwhere(got[k] == FILL)
        assert not miss.size, f"{what}: {len(miss)} of {got[k].size} words of frame {k} were never written, the first at " \
                              f"(frame {k}, row {int(miss[0][0])}, word {int(miss[0][1])})"
    for k in range(n):
        bad = np.argwhere(got[k] != want[k])
        if bad.size:
            y, x = (int(v) for v in bad[0])
            raise AssertionError(f"{what}: {len(bad)} of {got[k].size} words of frame {k} differ from the oracle, the first "
                                 f"at (frame {k}, row {y}, word {x}): {got[k].view(np.float32)[y, x]!r} oracle "
                                 f"{want[k].view(np.float32)[y, x]!r}")
    assert outside, f"{what}: {outside}"


def held_frames(what, buf, refs):
    """a case's three assertions on a GuardedFrames a call has written (the caller has synchronised): (a) every frame
    is the oracle's bit for bit, (b) no word of a frame is still the fill word, (c) no word of the guards, the lead,
    the rows' padding or the gaps was touched"""
    check_frames(what, buf.frames(), buf.outside(), refs)


def untouched(what, buf):
    """a call that has nothing to write: frames and everything around them still hold the fill"""
    outside = buf.outside()
    written = int((buf.frames() != FILL).sum())
    print(f"{what}: touched outside {outside.count}, frame words written {written}")
    assert outside, f"{what}: {outside}"
    assert written == 0, f"{what}: {written} words of the frames were written"
