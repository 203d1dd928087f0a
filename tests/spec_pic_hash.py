"""Decoded picture hash SEI (payload type 132, H.274 / H.266 Annex D) restated in numpy / hashlib for this project's sample layout:
uint16 words, two bytes per sample (bit depth 10), the whole decoded picture at its coded size, each plane on its own.

The byte string of a plane is its samples in raster order, low byte then high byte.  MD5: RFC 1321 over it.  CRC: 16-bit register
from 0xFFFF, polynomial 0x1021, every bit most significant bit of a byte first, 16 closing steps with bit 0 (crc_literal; crc() is the
standard library's table form of the same polynomial, started at 0xFFFF x^16 mod P = 0x1D0F).  Checksum: the masked byte sum modulo 2^32.

No implementation of this SEI was at hand when this was written: VECTORS below was computed from the text above, and the tests
(tests/test_pic_hash_cpu.py) hold the restatement to it."""
import binascii
import hashlib

import numpy as np

MD5, CRC, CHECKSUM = 0, 1, 2
VALUE_BYTES = {MD5: 16, CRC: 2, CHECKSUM: 4}


def plane_bytes(p: np.ndarray) -> bytes:
    return np.ascontiguousarray(p, dtype=np.uint16).astype("<u2").tobytes()


def crc_literal(data: bytes) -> int:
    """the definition, bit by bit"""
    crc = 0xFFFF
    for byte in data:
        for k in range(7, -1, -1):
            top = crc >> 15
            crc = ((crc << 1) | ((byte >> k) & 1)) & 0xFFFF
            if top:
                crc ^= 0x1021
    for _ in range(16):
        top = crc >> 15
        crc = (crc << 1) & 0xFFFF
        if top:
            crc ^= 0x1021
    return crc


def crc(data: bytes) -> int:
    return binascii.crc_hqx(data, 0x1D0F)


def checksum(p: np.ndarray) -> int:
    h, w = p.shape
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    m = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8)
    s = p.astype(np.int64)
    return int((((s & 0xFF) ^ m) + ((s >> 8) ^ m)).sum() & 0xFFFFFFFF)


def plane_value(method: int, p: np.ndarray) -> bytes:
    """the bytes of one plane's value as they stand in the SEI payload"""
    if method == MD5:
        return hashlib.md5(plane_bytes(p)).digest()
    if method == CRC:
        return crc(plane_bytes(p)).to_bytes(2, "big")
    return checksum(p).to_bytes(4, "big")


def picture_hash(method: int, planes, n_planes: int = 3) -> list:
    return [plane_value(method, planes[c]) for c in range(n_planes)]


def sei_payload(method: int, values: list) -> bytes:
    """dph_sei_hash_type u(8), dph_sei_single_component_flag u(1), 7 reserved bits, the values"""
    return bytes([method, 0x80 if len(values) == 1 else 0x00]) + b"".join(values)


def formula_picture(w: int, h: int):
    """s(x, y, c) = (37x + 101y + 7xy + 13c + ((x ^ y) << 3)) & 1023; luma w x h, chroma half of each"""
    def plane(pw, ph, c):
        x, y = np.arange(pw, dtype=np.int64)[None, :], np.arange(ph, dtype=np.int64)[:, None]
        return ((37 * x + 101 * y + 7 * x * y + 13 * c + ((x ^ y) << 3)) & 1023).astype(np.uint16)
    return plane(w, h, 0), plane(w // 2, h // 2, 1), plane(w // 2, h // 2, 2)


# luma size -> (CRC Y / Cb / Cr, checksum Y / Cb / Cr, MD5 Y) of formula_picture
VECTORS = {
    (8, 8): (("e55b", "f7bd", "5c5b"), ("00001ee1", "00000794", "0000085c"), "a91c7749a0e42e7239fcae6fe49af8ec"),
    (24, 8): (("6cee", "aa8e", "b34e"), ("0000696e", "00001a27", "0000198a"), "add3795b4791364bb3eb949be76768f5"),
    (72, 40): (("77d5", "b12f", "458f"), ("0007403a", "0001a5cd", "00019ea0"), "7ce24f75b803002a905dbe9177b49457"),
    (520, 264): (("fd3d", "9ee0", "e37c"), ("0215d6af", "00857bc2", "008515bf"), "52f5e941ffc9cbec15ab67395442611c"),
}
