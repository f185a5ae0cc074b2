"""A stand-in for the ``bitarray`` package, for the fixture generators only (tests/golden/make_golden_streams.py).

The reference's step 8 uses ten operations of ``bitarray.bitarray``: construction (empty or from a '01' string), ``+``,
``extend``, ``append``, ``len``, slicing, ``to01``, ``tobytes`` and ``frombytes``.  They are written here from the
package's documented behaviour, on a plain list of booleans:
  * bits are numbered from the most significant bit of each byte (the package's default, endian 'big');
  * ``tobytes`` fills the last byte with zero bits; ``frombytes`` appends 8 bits per byte;
  * a slice past the end comes back short, as a list slice does; an index returns one bit as an int;
  * ``extend`` takes a bitarray, a '01' string or an iterable of booleans; ``append`` takes the truth value of its
    argument.

This module imports nothing, shares no code with the product's ``util.Bits`` and is imported by no product file
(tests/test_bitarray_standin.py checks all three, and every operation against a str/int model).
"""


class bitarray:                                              # noqa: N801  (the package's own spelling)
    def __init__(self, initial=None):
        self._bits = []
        if initial is not None:
            self.extend(initial)

    def __len__(self):
        return len(self._bits)

    def __iter__(self):
        return iter(int(b) for b in self._bits)

    def __eq__(self, other):
        return isinstance(other, bitarray) and self._bits == other._bits

    def __repr__(self):
        return "bitarray('%s')" % self.to01()

    def __getitem__(self, key):
        if isinstance(key, slice):
            out = bitarray()
            out._bits = self._bits[key]
            return out
        return int(self._bits[key])

    def __add__(self, other):
        out = bitarray()
        out._bits = list(self._bits)
        out.extend(other)
        return out

    def append(self, bit):
        self._bits.append(bool(bit))

    def extend(self, other):
        if isinstance(other, bitarray):
            self._bits.extend(other._bits)
        elif isinstance(other, str):
            if other.strip("01"):
                raise ValueError("expected '0' or '1' in %r" % other)
            self._bits.extend(c == "1" for c in other)
        else:
            self._bits.extend(bool(b) for b in other)

    def to01(self):
        return "".join("1" if b else "0" for b in self._bits)

    def tobytes(self):
        bits = self._bits + [False] * (-len(self._bits) % 8)
        out = bytearray()
        for i in range(0, len(bits), 8):
            byte = 0
            for b in bits[i:i + 8]:
                byte = (byte << 1) | int(b)
            out.append(byte)
        return bytes(out)

    def frombytes(self, data):
        for byte in bytes(data):
            self._bits.extend(bool((byte >> shift) & 1) for shift in range(7, -1, -1))
