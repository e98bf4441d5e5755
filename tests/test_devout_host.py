"""The checks of tests/devout.py can fail: GuardedFrames (and Guarded) on device="cpu", where one word at a time is
poked into every kind of place a kernel must not write - the front guard, the lead, a row's padding, a gap, what lies
behind the last frame - and outside() must report exactly that word at its (frame, row, column); where one frame
word is left unwritten and assertion (b) must name it; and where nothing is wrong and everything must hold. The
addresses are worked out here from the layout's description, not by the class under test:

    GUARD + lead words | n frames | GUARD words,  a frame: rows x (row_units + pad) words, then gap words

No GPU is needed, and no kernel is broken on purpose to show that the GPU tests of tests/test_gpu_batch_bounds.py
and tests/test_gpu_render_bounds.py would notice."""
import numpy as np
import pytest

import devout
from devout import FILL, GUARD

ROWS, UNITS = 5, 7          # 7 words: 2 pixels of 3 channels and one more word, so no stride here is a multiple of another
POKE = 0x3F800000           # 1.0f


class Layout:
    """the addresses, from the description above"""

    def __init__(self, n, pad, lead, gap):
        self.n, self.pad, self.lead, self.gap = n, pad, lead, gap
        self.stride = UNITS + pad
        self.frame_stride = ROWS * self.stride + gap
        self.first = GUARD + lead
        self.total = self.first + n * self.frame_stride + GUARD

    def word(self, frame, row, col):
        return self.first + frame * self.frame_stride + row * self.stride + col

    def frame_words(self):
        f, r, c = np.meshgrid(np.arange(self.n), np.arange(ROWS), np.arange(UNITS), indexing="ij")
        return self.word(f, r, c)


def written(lay):
    """a buffer whose frames hold known finite floats, everything else the fill; (buffer, the frames as float32)"""
    buf = devout.GuardedFrames(lay.n, ROWS, UNITS, lay.pad, lay.lead, lay.gap, device="cpu")
    assert buf.buf.numel() == lay.total and buf.buf.device.type == "cpu"
    assert (buf.buf.numpy() == FILL).all()
    want = (np.arange(lay.n * ROWS * UNITS, dtype=np.float32) * np.float32(0.25) + np.float32(1.5)).reshape(lay.n, ROWS, UNITS)
    buf.buf.numpy()[lay.frame_words()] = want.view(np.int32)
    return buf, want


def pokes(lay):
    """(what, address, (frame, row, column)) of one word in each kind of place outside the rows"""
    mid, last = ROWS // 2, lay.n - 1
    out = [("the last word of the front guard", GUARD - 1, (0,) + divmod(-lay.lead - 1, lay.stride)),
           ("the word behind the last frame's last row", lay.word(last, ROWS, 0), (last, ROWS, 0)),
           ("the buffer's last word", lay.total - 1, (last,) + divmod(ROWS * lay.stride + lay.gap + GUARD - 1, lay.stride))]
    if lay.lead:
        out.append(("a lead word", GUARD, (0,) + divmod(-lay.lead, lay.stride)))
    if lay.pad:
        for f in sorted({0, last}):
            out.append((f"the first padding word of row {mid} of frame {f}", lay.word(f, mid, UNITS), (f, mid, UNITS)))
    if lay.gap:
        for f in sorted({0, last}):
            a = lay.word(f, ROWS, 0)
            if f != last:           # the last frame's is the word behind its last row, above
                out.append((f"the first word of the gap behind frame {f}", a, (f, ROWS, 0)))
            out.append((f"the last word of the gap behind frame {f}", a + lay.gap - 1,
                        (f, ROWS + (lay.gap - 1) // lay.stride, (lay.gap - 1) % lay.stride)))
        out.append(("the first word of the back guard", lay.total - GUARD,
                    (last, ROWS + lay.gap // lay.stride, lay.gap % lay.stride)))
    return out


LAYOUTS = [(n, pad, lead, gap) for n in (1, 3) for pad in (0, 1, 5) for lead in (0, 1) for gap in (0, 7)]


@pytest.mark.parametrize("n,pad,lead,gap", LAYOUTS)
def test_a_clean_buffer_holds(n, pad, lead, gap):
    lay = Layout(n, pad, lead, gap)
    buf, want = written(lay)
    assert buf.stride_bytes == 4 * lay.stride and buf.frame_stride_bytes == 4 * lay.frame_stride
    base = buf.buf.data_ptr()
    assert buf.ptr() == base + 4 * lay.first and buf.ptr(n - 1, 2) == base + 4 * lay.word(n - 1, 2, 0)
    outside = buf.outside()
    assert outside and outside.count == 0 and "nothing" in str(outside)
    got = buf.frames()
    assert got.dtype == np.uint32 and got.shape == (n, ROWS, UNITS)
    assert (got == want.view(np.uint32)).all()
    # the references may come as pixels and channels
    devout.check_frames("clean", got, outside, [w.reshape(ROWS, 1, UNITS) for w in want])
    devout.held_frames("clean", buf, list(want))


@pytest.mark.parametrize("n,pad,lead,gap", LAYOUTS)
def test_a_fresh_buffer_is_untouched_and_a_written_one_is_not(n, pad, lead, gap):
    lay = Layout(n, pad, lead, gap)
    buf = devout.GuardedFrames(n, ROWS, UNITS, pad, lead, gap, device="cpu")
    devout.untouched("fresh", buf)
    assert (buf.frames() == FILL).all()
    buf.buf[lay.word(n - 1, ROWS - 1, UNITS - 1)] = POKE
    with pytest.raises(AssertionError, match="1 words of the frames were written"):
        devout.untouched("one frame word", buf)


@pytest.mark.parametrize("n,pad,lead,gap", LAYOUTS)
def test_every_poked_word_is_reported_at_its_place(n, pad, lead, gap):
    lay = Layout(n, pad, lead, gap)
    kinds = pokes(lay)
    assert len(kinds) == 3 + bool(lead) + (1 + (n > 1)) * (bool(pad) + bool(gap)) + (n > 1) * bool(gap) + bool(gap)
    assert len({a for _, a, _ in kinds}) == len(kinds), "the poked words are different words"
    for what, address, place in kinds:
        buf, want = written(lay)
        assert address not in lay.frame_words()
        buf.buf[address] = POKE
        outside = buf.outside()
        assert not outside and outside.count == 1, f"{what}: {outside}"
        assert outside.first == place, f"{what}: reported at {outside.first}, poked at {place}"
        assert buf.where(address) == place
        assert f"(frame {place[0]}, row {place[1]}, column {place[2]})" in str(outside)
        assert (buf.frames() == want.view(np.uint32)).all(), f"{what}: frames() reads outside the rows"
        with pytest.raises(AssertionError, match="1 words outside the frames' rows were written"):
            devout.held_frames(what, buf, list(want))
        with pytest.raises(AssertionError, match="1 words outside"):
            devout.untouched(what, devout_fresh_with(lay, address))


def devout_fresh_with(lay, address):
    buf = devout.GuardedFrames(lay.n, ROWS, UNITS, lay.pad, lay.lead, lay.gap, device="cpu")
    buf.buf[address] = POKE
    return buf


@pytest.mark.parametrize("n,pad,lead,gap", LAYOUTS)
def test_the_first_of_several_is_the_lowest_address(n, pad, lead, gap):
    """one word in every kind of place at once: all are counted, the front guard's is named"""
    lay = Layout(n, pad, lead, gap)
    kinds = pokes(lay)
    buf, want = written(lay)
    for _, address, _ in kinds:
        buf.buf[address] = POKE
    outside = buf.outside()
    assert outside.count == len(kinds) and outside.first == min(kinds, key=lambda k: k[1])[2]
    # without the front guard's and the lead's: the next one up
    buf.buf[GUARD - 1] = FILL
    if lead:
        buf.buf[GUARD] = FILL
    rest = [k for k in kinds if k[1] > GUARD]
    outside = buf.outside()
    assert outside.count == len(rest) and outside.first == min(rest, key=lambda k: k[1])[2]
    assert (buf.frames() == want.view(np.uint32)).all()


@pytest.mark.parametrize("n,pad,lead,gap", LAYOUTS)
def test_an_unwritten_frame_word_is_named(n, pad, lead, gap):
    lay = Layout(n, pad, lead, gap)
    for f, r, c in {(0, 0, 0), (n - 1, ROWS - 1, UNITS - 1), (n // 2, 2, 3)}:
        buf, want = written(lay)
        buf.buf[lay.word(f, r, c)] = FILL
        assert buf.outside(), "a frame word is not outside"
        with pytest.raises(AssertionError, match=rf"1 of {ROWS * UNITS} words of frame {f} were never written, the first at "
                                                 rf"\(frame {f}, row {r}, word {c}\)"):
            devout.held_frames("unwritten", buf, list(want))


def test_a_wrong_frame_word_and_a_wrong_frame_order_are_named():
    lay = Layout(3, 1, 1, 7)
    buf, want = written(lay)
    buf.buf[lay.word(1, 4, 6)] = POKE
    with pytest.raises(AssertionError, match=r"1 of 35 words of frame 1 differ from the oracle, the first at \(frame 1, row 4, word 6\)"):
        devout.held_frames("wrong word", buf, list(want))
    buf, want = written(lay)
    with pytest.raises(AssertionError, match="words of frame 0 differ"):
        devout.held_frames("frames swapped", buf, [want[1], want[0], want[2]])
    with pytest.raises(AssertionError):
        devout.held_frames("a frame short", buf, list(want[:2]))


# ---- Guarded: the single frame of tests/test_gpu_render_bounds.py, the same way ---------------------------------
@pytest.mark.parametrize("pad", [0, 1, 5])
@pytest.mark.parametrize("lead", [0, 1])
def test_guarded_single_frame(pad, lead):
    stride, first = UNITS + pad, GUARD + lead
    total = first + ROWS * stride + GUARD

    def fresh():
        buf = devout.Guarded(ROWS, UNITS, pad, lead, device="cpu")
        assert buf.buf.numel() == total
        want = (np.arange(ROWS * UNITS, dtype=np.float32) + np.float32(0.5)).reshape(ROWS, UNITS)
        r, c = np.meshgrid(np.arange(ROWS), np.arange(UNITS), indexing="ij")
        buf.buf.numpy()[first + r * stride + c] = want.view(np.int32)
        return buf, want

    buf, want = fresh()
    assert buf.outside() and (buf.frame() == want.view(np.uint32)).all()
    devout.check("clean", want.copy(), buf.outside(), want)
    kinds = [(GUARD - 1, divmod(-lead - 1, stride)), (first + ROWS * stride, (ROWS, 0)), (total - 1, divmod(ROWS * stride + GUARD - 1, stride))]
    if lead:
        kinds.append((GUARD, divmod(-lead, stride)))
    if pad:
        kinds.append((first + 2 * stride + UNITS, (2, UNITS)))
    for address, place in kinds:
        buf, want = fresh()
        buf.buf[address] = POKE
        outside = buf.outside()
        assert not outside and outside.count == 1 and tuple(outside.first) == place, (address, outside.first, place)
        assert (buf.frame() == want.view(np.uint32)).all()
        with pytest.raises(AssertionError, match="outside the rows were written"):
            devout.check("poked", want.copy(), outside, want)
    buf, want = fresh()
    buf.buf[first + 3 * stride + 4] = FILL
    got = buf.frame().view(np.float32)
    with pytest.raises(AssertionError, match=r"1 of 35 words of the frame were never written, the first at \(3, 4\)"):
        devout.check("unwritten", got, buf.outside(), want)
