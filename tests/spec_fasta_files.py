"""The rules of the reference FASTA parser as a plain loop over lines (no NumPy masks): what
`snp_kmer_finder.read_fasta_records` (the host route) and `fasta_files` (the device route) must both give.

  header   a line that begins with '>' (so a '>' at byte 0 or right behind a '\\n'; any other '>' is a letter)
  name     the first word of the header line behind the '>', split as bytes.split() splits; '' when there is no word;
           decoded as ASCII with 'replace'
  body     every byte of the lines that follow, up to the next header, except the bytes 10 and 13
  before   bytes before the first header belong to no record
  twice    of records that share a name the first is the one meant
"""


def records(data):
    """(found, bodies): every header's name in file order, and name -> bytes of the first record of that name."""
    found, bodies, body = [], {}, None
    at = 0
    while at < len(data):
        end = data.find(b"\n", at)
        end = len(data) if end < 0 else end + 1
        line = data[at:end]
        at = end
        if line[:1] == b">":
            words = line[1:].split()
            name = words[0].decode("ascii", "replace") if words else ""
            found.append(name)
            body = None
            if name not in bodies:
                body = bodies[name] = bytearray()
        elif body is not None:
            for c in line:
                if c != 10 and c != 13:
                    body.append(c)
    return found, {n: bytes(b) for n, b in bodies.items()}


def distinct(found):
    """Every distinct name, in file order: what the device route takes `names=None` to mean."""
    out = []
    for n in found:
        if n not in out:
            out.append(n)
    return out


def read(data, names=None, file_name="<spec>"):
    """(names, bodies list[bytes], found); KeyError with read_fasta_records' text for a name that is not there.  names
    None: every header's name in file order, as read_fasta_records has it (a name that occurs twice is listed twice, both
    times with the first record's letters)."""
    found, bodies = records(data)
    names = list(found if names is None else names)
    for n in names:
        if n not in bodies:
            raise KeyError("no record %r in %s (records: %s)" % (n, file_name, ", ".join(found)))
    return names, [bodies[n] for n in names], found
