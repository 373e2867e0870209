"""VCF buffers for the device parser (csrc/gki_vcf_parse.hip), plain bytes: the smallest shapes at which each kernel can
still go wrong.  GOOD: buffers VariantArrays.from_vcf reads; BAD: buffers with a bad data line, with (data line, kind)."""
T = 4096            # csrc/gki_text_lines.h PARSE_TILE: the bytes one workgroup of the line-end pass scans

HEADER = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def line(chrom, pos, ref=b"A", alt=b"C", rest=b".\t.\t."):
    return b"\t".join([chrom, b"%d" % pos, b".", ref, alt, rest]) + b"\n"


def padded_to(n, byte_at=None, at=None):
    """A buffer of exactly n bytes of two-chromosome data lines; with `at`, byte `at` is `byte_at` ('\\n' or a tab): the
    line that crosses it has an INFO field sized so that its end falls there, or a CHROM so long that its first tab does."""
    out, pos = bytearray(HEADER), 1
    target = n if at is None else at
    while True:
        chrom = b"chr1" if pos < 40 else b"chr10"
        head = b"%s\t%d\t.\tA\tC\t.\t." % (chrom, pos)               # then "\t" + INFO + "\n"
        if len(out) + len(head) + 60 > target:
            break
        out += head + b"\tDP=%d\n" % pos
        pos += 1
    chrom = b"chr10"
    if at is None:
        out += b"%s\t%d\t.\tA\tC\t.\t.\t" % (chrom, pos)
        out += b"X" * (n - len(out) - 1) + b"\n"
    elif byte_at == b"\n":
        out += b"%s\t%d\t.\tA\tC\t.\t.\t" % (chrom, pos)
        out += b"X" * (at - len(out)) + b"\n"
    else:                                                            # the tab behind CHROM at byte `at`: a long name
        out += b"c" * (at - len(out)) + b"\t%d\t.\tA\tC\n" % pos
    if at is not None:
        assert out[at:at + 1] == byte_at
        while len(out) + 60 < n:
            pos += 1
            out += b"chrX\t%d\t.\tAC\tA\t.\t.\t.\n" % pos
        pos += 1
        tail = b"chrX\t%d\t.\tG\tT\t.\t.\t" % pos
        out += tail + b"Y" * (n - len(out) - len(tail) - 1) + b"\n"
    assert len(out) == n
    return bytes(out)


def genotype_line(chrom, pos, n_bytes):
    """A data line of at least n_bytes bytes: FORMAT GT and as many 0|1 columns as it takes."""
    n_samples = n_bytes // 4 + 1
    return b"%s\t%d\t.\tA\tC\t.\tPASS\t.\tGT" % (chrom, pos) + b"\t0|1" * n_samples + b"\n"


GOOD = {
    "empty": b"",
    "headers_only": HEADER,
    "headers_only_open_end": HEADER[:-1],
    "plain": HEADER + line(b"1", 10) + line(b"1", 20, b"AC", b"A") + line(b"2", 5),
    "blank_lines": HEADER + b"\n" + line(b"1", 10) + b" \t \t\n" + line(b"1", 11) + b"\n\n",
    "crlf": (HEADER + line(b"1", 10) + b"\n" + line(b"1", 20, b"A", b"ACG") + line(b"2", 7)).replace(b"\n", b"\r\n"),
    "open_end": HEADER + line(b"1", 10) + line(b"3", 30)[:-1],
    "open_end_crlf": HEADER + line(b"1", 10) + b"3\t30\t.\tA\tC\r",
    "field_counts": b"1\t10\n1\t11\t.\tA\n1\t12\t.\tA\tC\n1\t13\t.\tA\tC\t.\t.\t.\n1\t14\t\n1\t15\t.\tA\t\n",
    "ref_alt_pairs": b"".join(line(b"1", 10 + i, r, a) for i, (r, a) in enumerate(
        [(b"A", b"C"), (b"AC", b"A"), (b"A", b"ACG"), (b"A", b"C,G"), (b"A", b"<DEL>"), (b"A", b"")])),
    "alt_ends_the_line": b"1\t10\t.\tA\tC\n1\t11\t.\tA\tCG\n1\t12\t.\tA\t\n1\t13\t.\tA\tC\r\n",
    "empty_chrom": b"\t10\t.\tA\tC\n\t11\t.\tA\tC\n1\t12\t.\tA\tC\n\t13\t.\tA\tC\n",
    "pos_forms": b"1\t007\t.\tA\tC\n1\t123456789012345678\t.\tA\tC\n1\t0\n1\t000000000000000000\n",
    "prefix_names": b"".join(line(c, 10 + i) for i, c in enumerate(
        [b"1", b"1", b"11", b"11", b"1", b"chr1", b"chr10", b"chr10", b"chr1", b"chr1"])),
    "return_to_a_name": line(b"1", 1) + line(b"2", 2) + line(b"2", 3) + line(b"1", 4),
    "one_run": b"".join(line(b"chr7", i + 1) for i in range(300)),
    "name_with_blanks": b" 1\t5\t.\tA\tC\n 1\t6\t.\tA\tC\nchr 2 \t7\t.\tA\tC\n",
    "hash_inside": b"1#\t5\t.\tA\tC\n #\t6\t.\tA\tC\n",
    "genotypes_over_a_tile": HEADER + line(b"1", 5) + genotype_line(b"1", 6, T + 100) + line(b"2", 7),
    "genotypes_over_64k": HEADER + genotype_line(b"1", 6, 65536 + 100) + genotype_line(b"2", 8, 70000) + line(b"2", 9),
    "bytes_4095": padded_to(T - 1),
    "bytes_4096": padded_to(T),
    "bytes_4097": padded_to(T + 1),
    "newline_at_4095": padded_to(2 * T + 5, b"\n", T - 1),
    "newline_at_4096": padded_to(2 * T + 5, b"\n", T),
    "tab_at_4096": padded_to(2 * T + 5, b"\t", T),
    "many_lines": HEADER + b"".join(line(b"%d" % (1 + i // 1500), i + 1, b"A" * (1 + i % 2)) for i in range(5000)),
}

# buffers passed at a device address that is not 16-byte aligned too (a view one byte into a DeviceArray)
UNALIGNED = ("plain", "crlf", "prefix_names", "genotypes_over_a_tile", "newline_at_4096", "bytes_4097")

BAD = {
    "no_tab_second_line": (b"1\t10\nxx\n", 1, 1),
    "letter_in_pos": (b"1\t1x\n", 0, 2),
    "signed_pos": (b"1\t+3\n", 0, 2),
    "pos_of_19_digits": (b"1\t1234567890123456789\n", 0, 2),
    "empty_pos": (b"1\t\t.\tA\tC\n", 0, 2),
    "blank_in_pos": (HEADER + line(b"1", 4) + b"1\t 5\n", 1, 2),
    "underscore_in_pos": (b"1\t1_0\n", 0, 2),
    "two_bad_lines": (line(b"1", 1) + b"1\tx\n" + b"yy\n", 1, 2),
    "bad_after_many": (b"".join(line(b"1", i + 1) for i in range(3000)) + b"zz\n" + line(b"1", 9), 3000, 1),
}
