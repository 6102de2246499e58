"""Device buffers between guard bands.  TEST INFRASTRUCTURE (no GPU, and no torch, at import).

The device has no address sanitizer, so a kernel that stores one row past its frame, or whose dead lanes store, corrupts whatever was
allocated next and no comparison of the frame sees it.  Here every buffer a kernel is handed lies in the MIDDLE of one device allocation,
between two bands of SENTINEL words (tests/stream_harness.py's value: a NaN with a payload that no arithmetic produces):

    | band: SENTINEL ... | body: n words | band: SENTINEL ... |

* an OUTPUT's body is pre-filled with the sentinel too: after the call both bands still hold it everywhere (the failure names the
  buffer and the first touched offset), no body word holds it any more (the call must write every word), and the body is the reference;
* an INPUT's body holds the data.  The sentinel is a NaN: an out-of-frame read that reaches the arithmetic poisons a pixel and fails
  the comparison of the outputs.  After the call the body is the data still, bit for bit, and so are the bands;
* an IN-OUT buffer (the adaptive update's moments and state, tone mapping's record, a frame mapped in place) is an input whose body is
  then compared like an output's;
* a one-word COUNT lies in the middle of a block of its own, pre-set to a non-zero value: counts are overwritten, not added to.

A band is band_words(...) long: at least 256 words, at least a whole row of tiles of the frame — every store the dead lanes of a
rounded-up last tile row could make, and a margin — and a multiple of 4 words, so that a body keeps the 16-byte alignment of its block
(the guide's two float4s per pixel, tone mapping's 16-byte loads)."""
from __future__ import annotations

import numpy as np

SENTINEL = 0x7FC0BEEF  # a NaN with a payload: an untouched float keeps these bits
COUNT_PRESET = 12345  # what a one-word count holds before the call: not 0, so a count that is added to shows
MIN_BAND = 256


def band_words(width: int, tile_h: int, words_per_pixel: int) -> int:
    """The length of one band around a buffer of `words_per_pixel` words a pixel of a frame `width` wide, for a kernel whose tiles are
    `tile_h` rows high (1 for a linear kernel): max(256, tile_h x width x words_per_pixel), rounded up to 4 words."""
    assert width >= 1 and tile_h >= 1 and words_per_pixel >= 1
    return -(-max(MIN_BAND, tile_h * width * words_per_pixel) // 4) * 4


def as_words(array) -> np.ndarray:
    """The 32-bit words of a float32, int32 or uint32 array, flat, as uint32 (a copy)."""
    array = np.ascontiguousarray(array)
    assert array.dtype.itemsize == 4, array.dtype
    return array.reshape(-1).view(np.uint32).copy()


def first_touched(words: np.ndarray):
    """The offset of the first word of a band that no longer holds the sentinel, or None."""
    touched = np.flatnonzero(words != np.uint32(SENTINEL))
    return int(touched[0]) if len(touched) else None


def check_bands(name: str, words: np.ndarray, band: int) -> np.ndarray:
    """`words`: a whole block as it came back from the device.  Asserts both bands untouched and returns the body (a view)."""
    assert len(words) >= 2 * band
    below, above = first_touched(words[:band]), first_touched(words[len(words) - band :])
    assert below is None, f"{name}: the band BELOW the buffer was written, first at word {below - band} from the buffer's start (0x{int(words[below]):08x})"
    assert above is None, f"{name}: the band ABOVE the buffer was written, first at word {above} past the buffer's end (0x{int(words[len(words) - band + above]):08x})"
    return words[band : len(words) - band]


class Buffer:
    """One guarded block.  `ptr` is the body's device address; `body()` fetches the block (once), checks the bands, returns the body."""

    def __init__(self, name: str, n: int, band: int, device: str, content=None):
        import torch

        assert n >= 1 and band >= MIN_BAND and band % 4 == 0
        self.name, self.n, self.band = name, n, band
        host = np.full(n + 2 * band, SENTINEL, dtype=np.uint32)
        self.before = None
        if content is not None:
            self.before = as_words(content)
            assert len(self.before) == n, (name, len(self.before), n)
            host[band : band + n] = self.before
        self.tensor = torch.from_numpy(host.view(np.int32)).to(device)
        self.ptr = self.tensor.data_ptr() + 4 * band
        assert self.ptr % 16 == 0, name
        self._body = None

    def body(self) -> np.ndarray:
        if self._body is None:
            self._body = check_bands(self.name, self.tensor.cpu().numpy().view(np.uint32), self.band)
        return self._body

    def assert_unchanged(self):
        """An input: the body is what was put there, bit for bit."""
        differing = np.flatnonzero(self.body() != self.before)
        assert not len(differing), f"{self.name}: an input was written, first at word {int(differing[0])}"

    def assert_is(self, want, what: str = "", every_word_written: bool = True):
        """An output: every word written (none holds the sentinel), and the body is `want`'s words."""
        got, want = self.body(), as_words(want)
        assert len(want) == self.n, (self.name, len(want), self.n)
        if every_word_written:
            unwritten = np.flatnonzero(got == np.uint32(SENTINEL))
            assert not len(unwritten), f"{what}: {self.name}: {len(unwritten)} of {self.n} words were never written, first word {int(unwritten[0])}"
        differing = np.flatnonzero(got != want)
        assert not len(differing), f"{what}: {self.name}: {len(differing)} of {self.n} words differ from the reference, first word {int(differing[0])}: 0x{int(got[differing[0]]):08x} for 0x{int(want[differing[0]]):08x}"


class Arena:
    """The guarded buffers of ONE call.  Make them, pass their `.ptr`s, then `check()`: every band of every buffer and every input's
    body; the outputs are compared by the caller with `assert_is` / `count_is`."""

    def __init__(self, device: str, width: int, tile_h: int):
        self.device, self.width, self.tile_h = device, width, tile_h
        self.buffers, self.inputs = [], []

    def _band(self, words_per_pixel):
        return band_words(self.width, self.tile_h, words_per_pixel)

    def input(self, name: str, array, words_per_pixel: int) -> Buffer:
        b = Buffer(name, np.asarray(array).size, self._band(words_per_pixel), self.device, array)
        self.buffers.append(b), self.inputs.append(b)
        return b

    def inout(self, name: str, array, words_per_pixel: int) -> Buffer:
        b = Buffer(name, np.asarray(array).size, self._band(words_per_pixel), self.device, array)
        self.buffers.append(b)
        return b

    def output(self, name: str, pixels: int, words_per_pixel: int) -> Buffer:
        b = Buffer(name, pixels * words_per_pixel, self._band(words_per_pixel), self.device)
        self.buffers.append(b)
        return b

    def count(self, name: str) -> Buffer:
        b = Buffer(name, 1, MIN_BAND, self.device, np.array([COUNT_PRESET], dtype=np.uint32))
        self.buffers.append(b)
        return b

    def check(self):
        for b in self.buffers:
            b.body()
        for b in self.inputs:
            b.assert_unchanged()


def count_of(b: Buffer) -> int:
    return int(b.body()[0])
