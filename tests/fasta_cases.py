"""Reference FASTA texts for the record parser, built in code: CASES name -> bytes, SELECTIONS name -> lists of names to
ask for (beside None, every record), MISSING name -> a name the file does not have.

The sizes are the smallest at which the device kernels can go wrong: a lane owns 16 bytes, a wave 1024, a workgroup's
tile 4096 (csrc/gki_text_lines.h)."""
import numpy as np

LANE, WAVE, TILE = 16, 1024, 4096


def letters(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)[rng.integers(0, 10, size=n)].tobytes()


def wrapped(body, width=60, end=b"\n"):
    return b"".join(body[a:a + width] + end for a in range(0, len(body), width))


def header_at(offset):
    """A file whose second header's '>' is byte `offset`: the first record's body fills what is before it."""
    assert offset >= 5
    head = b">p\n" + letters(offset - 4, offset) + b"\n"
    assert len(head) == offset
    return head + b">q%d the rest\n" % offset + letters(40, offset + 1) + b"\nGATTACA\n"


def crlf_across(boundary):
    """CRLF line ends with one '\\r' as byte boundary - 1 and its '\\n' as byte boundary, and the pair the other way round
    (the '\\r' as byte 2 * boundary) further on."""
    text = b">c\r\n"
    text += letters(boundary - 1 - len(text), boundary) + b"\r\n"
    assert text[boundary - 1:boundary + 1] == b"\r\n"
    text += letters(2 * boundary - len(text), boundary + 1) + b"\r\n"
    assert text[2 * boundary:2 * boundary + 2] == b"\r\n"
    return text + b"ACGT\r\n>d\r\nTT\r\n"


def many_records():
    """Six records of lengths around the wrap width and the tile, wrapped at 60; record r3 is empty."""
    sizes = {"r0": 59, "r1": 60, "r2": 61, "r3": 0, "r4": 4200, "r5": 1}
    return b"".join(b">%s record %d\n" % (n.encode(), i) + wrapped(letters(size, 40 + i))
                    for i, (n, size) in enumerate(sizes.items()))


def _cases():
    c = {}
    # tile, wave and lane boundaries
    c["header_at_4095"] = header_at(TILE - 1)             # the '>' ends a tile, the name is in the next one
    for off in (LANE - 1, LANE, WAVE - 1, WAVE, TILE, 2 * TILE - 1):
        c["header_at_%d" % off] = header_at(off)
    c["header_line_over_two_tiles"] = b">long " + b"x" * (2 * TILE + 900) + b"\nACGT\n>b\nTT\n"    # tile 1 is all header
    c["name_over_two_tiles"] = b">s\nAC\n>" + b"n" * (2 * TILE + 100) + b"\nACGT\nGG\n"
    c["unwrapped_body"] = b">u\n" + letters(2 * TILE + 1, 1) + b"\n>v\nAC\n"
    c["unwrapped_last_record_open_end"] = b">t\nAC\n>u\n" + letters(2 * TILE + 77, 2)
    c["crlf_across_lanes"] = crlf_across(LANE)
    c["crlf_across_waves"] = crlf_across(WAVE)
    c["crlf_across_tiles"] = crlf_across(TILE)
    c["lone_cr_mid_line"] = b">l\nAC\rGT\nAA\r\rCC\n"
    # records and names
    c["two_headers_in_a_row"] = b">a\n>b\nAC\n>c\n>d\n"
    c["empty_lines_in_body"] = b">a\nAC\n\n\nGT\n\n>b\n\nTT\n"
    c["header_is_last_line_open_end"] = b">a\nAC\n>last"
    c["header_only_open_end"] = b">only"
    c["no_name"] = b">\nAC\n> desc\nGG\n"               # `>` alone: no word; `> desc`: the first word is desc
    c["no_word_at_all"] = b"> \t \nAC\n>\x0b\x0c\r\nGG\n"
    c["name_ended_by_separators"] = b">a\tx\nA\n>b\x0bx\nC\n>c\x0cx\nG\n>d\r\nT\n>e f\nN\n"
    c["name_is_the_whole_line"] = b">whole_line\nAC\n"
    c["name_not_ascii"] = b">caf\xc3\xa9 x\nAC\n>\xff\nGG\n"
    c["other_controls_are_name_bytes"] = b">a\x1cb\x00c d\nAC\n"        # 0x1C and 0 separate nothing in bytes.split()
    c["gt_inside_body_line"] = b">a\nAC>GT\n>b\nA>\n >c\nTT\n"
    c["blank_inside_body_line"] = b">a\nAC GT\n T\t\n"
    c["text_before_first_header"] = b"junk\nmore junk\r\n>a\nAC\n"
    c["no_header"] = b"ACGT\nACGT\n"
    c["only_line_ends"] = b"\n\r\n\n"
    c["empty_file"] = b""
    c["one_byte_header"] = b">"
    # selection
    c["name_twice"] = b">x\nAA\n>y\nCC\n>x\nGGGG\nGG\n>z\nT\n"
    c["empty_name_twice"] = b">\nAA\n> \nCCCC\n>y\nT\n"
    c["many_records"] = many_records()
    c["many_records_crlf_open_end"] = many_records().replace(b"\n", b"\r\n")[:-2]
    return c


CASES = _cases()
SELECTIONS = {
    "name_twice": [["x"], ["z", "x"], ["y"]],
    "empty_name_twice": [[""], ["y", ""]],
    "many_records": [["r4", "r1"], ["r5", "r3", "r0"], ["r2"], ["r1", "r1"]],
    "many_records_crlf_open_end": [["r5", "r2"]],
    "two_headers_in_a_row": [["d", "a"]],
    "header_at_4095": [["q4095"], ["q4095", "p"]],
    "no_name": [["desc"], [""]],
}
MISSING = {"many_records": "r9", "name_twice": "w", "no_header": "a", "empty_file": "a"}
# the cases the streamed tests cut into pieces: a record over many pieces, pieces that begin with a header, CRLF
PIECE_CASES = ("many_records", "many_records_crlf_open_end", "name_twice", "text_before_first_header", "header_at_4095")
