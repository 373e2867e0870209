"""Command-line drivers with the reference's sub-command and option names for the in-scope path
(command_line_interface.py:156-174 make_from_flat, :553-638 index, :640-667 find_critical_paths /
add_reverse_complements), writing the reference's .npz formats (flat_kmers.py:65-68,
collision_free_kmer_index.py:393-402).

    python -m graph_kmer_index_amd.command_line_interface index -g graph.npz -k 31 -o flat
    python -m graph_kmer_index_amd.command_line_interface make_from_flat -f flat -o index
    python -m graph_kmer_index_amd.command_line_interface make_unique_variant_kmers -g graph.npz -V variant_to_nodes.npz \
        -k 31 -i index.npz -p position_id -D True -v variants.vcf -o variant_kmers
    python -m graph_kmer_index_amd.command_line_interface sample_kmers_from_structural_variants -g graph.npz \
        -V variant_to_nodes.npz -k 31 -i index.npz -o sv_kmers
    python -m graph_kmer_index_amd.command_line_interface count_kmers -f linear_kmers.npz -o counter
    python -m graph_kmer_index_amd.command_line_interface sample_kmers_from_structural_variants -g graph.npz \
        -V variant_to_nodes.npz -k 31 -I counter.npz -o sv_kmers
    python -m graph_kmer_index_amd.command_line_interface merge_flat_kmers -f variant_kmers.npz,sv_kmers.npz -o all_variant_kmers
    python -m graph_kmer_index_amd.command_line_interface make_reverse -f variant_kmers.npz -o reverse
    python -m graph_kmer_index_amd.command_line_interface make -t 16 -s 1 -k 31 -r True -R ref.fa -n chr1 -G <size> -o linear_kmers
    python -m graph_kmer_index_amd.command_line_interface map -i index.npz -f reads.fq.gz -k 31 -o node_counts
    python -m graph_kmer_index_amd.command_line_interface make_graph -r ref.fa -v variants.vcf.gz -o graph -n chr1,chr2 -a genotypes
    python -m graph_kmer_index_amd.command_line_interface make_haplotype_matrix -v variants.vcf.gz -o haplotypes --planes True
    python -m graph_kmer_index_amd.command_line_interface make_haplotype_to_nodes -g graph.npz -V graph.variant_to_nodes.npz \
        -m haplotypes.npz -o haplotype_to_nodes
    python -m graph_kmer_index_amd.command_line_interface spell_haplotype -g graph.npz -V graph.variant_to_nodes.npz \
        -m haplotypes.npz -s 0 -o haplotype0.fa
    python -m graph_kmer_index_amd.command_line_interface haplotype_node_counts -g graph.npz -V graph.variant_to_nodes.npz \
        -m haplotypes.npz -i index.npz -k 31 -s 0,1,5 -o haplotype_counts [--route difference]
    python -m graph_kmer_index_amd.command_line_interface make_node_count_model -g graph.npz -V graph.variant_to_nodes.npz \
        -m haplotypes.npz -i index.npz -k 31 [-s 0,1,5] [-b 5] -o node_count_model
    python -m graph_kmer_index_amd.command_line_interface genotype -V graph.variant_to_nodes.npz -M node_count_model.npz \
        -c node_counts.npy -v variants.vcf.gz -o sample.vcf [-s name] [--coverage X] [--error 0.01] [--pseudo-count 1] [-L loglik] \
        [--compress none|bgzf|auto]
    python -m graph_kmer_index_amd.command_line_interface genotype -V graph.variant_to_nodes.npz -M node_count_model.npz \
        -c cohort_counts.npy | -c a.npy,b.npy,c.npy -v variants.vcf.gz -o cohort.vcf [-s a,b,c] [--coverage X | X,Y,Z] \
        [--batch-bytes N]
    python -m graph_kmer_index_amd.command_line_interface bgzf -i reads.fq -o reads.fq.gz [--block-size 65280] [--chunk-bytes N]

`-g` takes an obgraph file when obgraph is installed, else a GraphArrays .npz (GraphArrays.to_file).  `index -t N` runs
one process per GPU (at most N, at most the visible devices), each on its own range of critical-path numbers, and
concatenates the shards in rank order -- the reference's process pool over chunks (:575-614) with GPUs for workers.
"""
import argparse
import logging
import sys
import numpy as np

from . import _lib
from .collision_free_kmer_index import CollisionFreeKmerIndex
from .critical_graph_paths import CriticalGraphPaths
from .flat_kmers import FlatKmers
from .graph import GraphArrays
from .kmer_finder import DenseKmerFinder


def load_graph(file_name):
    try:
        return GraphArrays.from_file(file_name)                 # GraphArrays.to_file dump
    except (KeyError, ValueError, OSError):
        from obgraph import Graph                               # the reference's loader (needs obgraph installed)
        return GraphArrays.from_obgraph(Graph.from_file(file_name))


def load_critical_paths(file_name):
    if file_name is None:
        return None
    try:
        d = np.load(file_name if file_name.endswith(".npz") else file_name + ".npz")
        return CriticalGraphPaths(d["nodes"], d["offsets"])
    except (FileNotFoundError, KeyError, ValueError):
        from shared_memory_wrapper import from_file      # the reference's serialisation, when available
        return from_file(file_name)


def _bool(x):
    return bool(x) if not isinstance(x, str) else x.lower() not in ("", "0", "false", "no")


def index(args):
    if args.shard is None and max(1, args.n_threads) > 1:
        ranks = args.ranks or min(args.n_threads, max(1, _visible_devices()))
        if ranks > 1:
            return index_on_ranks(args, ranks)
        logging.info("-t %d: one device visible, one process" % args.n_threads)
    shard = None
    if args.shard is not None:                       # one rank of `index -t N`: its device FIRST -- the critical paths
                                                     # below are computed on the device and the graph upload is cached on
        shard = tuple(int(x) for x in args.shard.split("/"))     # the graph object: both must land on this rank's GPU
        _lib.check(_lib.load().gki_set_device(shard[0] % max(1, _lib.device_count())))
    graph = load_graph(args.graph)
    k = args.kmer_size
    cp = load_critical_paths(args.critical_graph_paths) or CriticalGraphPaths.from_graph(graph, k)
    whitelist = None
    if args.whitelist is not None:
        whitelist = CollisionFreeKmerIndex.from_file(args.whitelist)                      # :634 (`kmer in whitelist`)
    chunk = {}
    if shard is not None:                            # its range of critical-path numbers
        from .sharding import shard_range
        r, w = shard
        a, b = shard_range(GraphArrays.from_obgraph(graph), cp, r, w)
        chunk = dict(start_at_critical_path_number=a, stop_at_critical_path_number=b)
    finder = DenseKmerFinder(graph, k, critical_graph_paths=cp, max_variant_nodes=args.max_variant_nodes,
                             only_save_one_node_per_kmer=True, whitelist=whitelist, **chunk)      # :559-565
    with _lib.DeviceScope() as s:
        dflat = s.keep(finder.find_flat_on_device(split_layout=False))    # with a whitelist: membership probe + compaction in HBM
        finder.synchronize()
        if args.include_reverse_complement and args.shard is None:                        # :616-620, still in HBM
            from .flat_kmers import DeviceFlatKmers
            both = s.keep(DeviceFlatKmers.from_multiple_flat_kmers([dflat, s.keep(dflat.get_reverse_complement_flat_kmers(k))]))
            dflat.free()                             # early: one copy of the records is enough from here
            dflat = both
        flat = dflat.to_flat_kmers()
    logging.info("N kmers in flat kmers: %d" % len(flat._hashes))
    flat.to_file(args.out_file_name)


def _visible_devices():
    return _lib.device_count()


def index_on_ranks(args, ranks):
    """`index -t N` (command_line_interface.py:575-614 spreads n_threads * 20 chunks of critical-path numbers over a
    process pool and concatenates the results in chunk order): here one process per GPU, each taking one contiguous
    range of critical-path numbers balanced by bases (sharding.shard_range -- no k-window crosses a critical point, so
    the ranges need no halo), writing its FlatKmers shard; this process concatenates the shards in rank order
    (flat_kmers.py:71-90) and adds the reverse complements afterwards like the reference (:616-620)."""
    import os
    import subprocess
    import tempfile
    k = args.kmer_size
    with tempfile.TemporaryDirectory(prefix="gki_index_") as tmp:
        procs = []
        for r in range(ranks):
            cmd = [sys.executable, "-m", "graph_kmer_index_amd.command_line_interface", "index", "-g", args.graph, "-k", str(k),
                   "-o", os.path.join(tmp, "shard_%d" % r), "-v", str(args.max_variant_nodes), "--shard", "%d/%d" % (r, ranks)]
            if args.critical_graph_paths:
                cmd += ["-c", args.critical_graph_paths]
            if args.whitelist:
                cmd += ["-w", args.whitelist]
            env = dict(os.environ)
            root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
            procs.append(subprocess.Popen(cmd, env=env))
        codes = [p.wait() for p in procs]
        if any(codes):
            raise RuntimeError("index: rank exit codes %s" % codes)
        flat = FlatKmers.from_multiple_flat_kmers([FlatKmers.from_file(os.path.join(tmp, "shard_%d" % r)) for r in range(ranks)])
    if args.include_reverse_complement:
        flat = FlatKmers.from_multiple_flat_kmers([flat, flat.get_reverse_complement_flat_kmers(k=k)])
    logging.info("N kmers in flat kmers: %d (from %d ranks)" % (len(flat._hashes), ranks))
    flat.to_file(args.out_file_name)


def make_from_flat(args):
    flat = FlatKmers.from_file(args.flat_index)
    if args.add_reverse_complements:
        flat = FlatKmers.from_multiple_flat_kmers([flat, flat.get_reverse_complement_flat_kmers(k=args.kmer_size)])
    if args.make_minimal:
        raise NotImplementedError("MinimalKmerIndex is out of scope (broken on NumPy >= 1.24 in the reference)")
    idx = CollisionFreeKmerIndex.from_flat_kmers(flat, modulo=args.hash_modulo, skip_frequencies=args.skip_frequencies,
                                                 skip_singletons=args.skip_singletons)
    idx.to_file(args.out_file_name)


def find_critical_paths(args):
    cp = CriticalGraphPaths.from_graph(load_graph(args.graph), args.kmer_size)
    cp._make_index()
    np.savez(args.out_file_name, nodes=cp.nodes, offsets=cp.offsets)


def add_reverse_complements(args):
    flat = FlatKmers.from_file(args.flat_kmers)
    FlatKmers.from_multiple_flat_kmers([flat, flat.get_reverse_complement_flat_kmers(k=args.kmer_size)]) \
        .to_file(args.out_file_name)


def make_reverse(args):
    """command_line_interface.py:177-181."""
    from .reverse_kmer_index import ReverseKmerIndex
    flat = FlatKmers.from_file(args.flat_index)
    ReverseKmerIndex.from_flat_kmers(flat).to_file(args.out_file_name)
    logging.info("Done. Wrote reverse index to file: %s" % args.out_file_name)


def load_position_id(file_name, graph):
    """-p: the reference's PositionId file (through shared_memory_wrapper when installed); None = the default position
    ids of the graph (exclusive cumulative node size)."""
    if file_name is None:
        return _DefaultPositionId(graph)
    from shared_memory_wrapper import from_file
    return from_file(file_name)


class _DefaultPositionId:
    def __init__(self, graph):
        self._base = GraphArrays.from_obgraph(graph).position_id_base()

    def get(self, nodes, offsets):
        return self._base[np.asarray(nodes, dtype=np.int64)] + np.asarray(offsets, dtype=np.int64)


def load_frequency_source(args, command):
    """-i: a CollisionFreeKmerIndex with frequencies; when it is absent, -I: a KmerCounter written by count_kmers
    (command_line_interface.py:308-310 of the reference)."""
    if args.kmer_index is not None:
        return CollisionFreeKmerIndex.from_file(args.kmer_index)
    if args.kmer_counter is None:
        raise ValueError("%s: -i (a CollisionFreeKmerIndex with frequencies) or -I (a KmerCounter from count_kmers) is "
                         "required" % command)
    from .kmer_counter import KmerCounter
    try:
        return KmerCounter.from_file(args.kmer_counter)
    except (FileNotFoundError, ValueError) as e:
        raise type(e)("%s: %s (a counter written by this package's count_kmers is expected; the reference's pickled "
                      "npstructures table given with -I is not supported)" % (command, e))


def count_kmers(args):
    """command_line_interface.py:670-681: the unique k-mers of a flat with their counts, every -s'th record taken."""
    from .kmer_counter import KmerCounter
    counter = KmerCounter.from_flat_kmersv2(FlatKmers.from_file(args.flat_kmers), args.modulo, args.subsample_ratio)
    counter.to_file(args.out_file_name)
    logging.info("Wrote counter of %d k-mers to %s" % (len(counter._kmers), args.out_file_name))


def make_kmer_frequencies(args):
    """command_line_interface.py:499-509."""
    from .kmer_frequency_index import KmerFrequencyIndex
    from .reference_kmer_index import ReferenceKmerIndex
    ref_kmers = ReferenceKmerIndex.from_file(args.reference_kmers)
    index = KmerFrequencyIndex.from_kmers(ref_kmers.kmers)
    index.to_file(args.out_file_name)
    logging.info("Wrote to file %s" % args.out_file_name)


def load_variants(args):
    """The VCF of `-v` as VariantArrays: `--vcf-parse host` reads the lines in Python (VariantArrays.from_vcf), `device`
    and `auto` parse them on the device, a `.gz` file inflated as `--inflate` says."""
    from .unique_variant_kmers import VariantArrays
    if args.vcf_parse == "host":
        return VariantArrays.from_vcf(args.vcf)
    return VariantArrays.from_vcf_on_device(args.vcf, inflate=args.inflate)


def make_unique_variant_kmers(args):
    """command_line_interface.py:299-389, dense path: one finder per `-c` chunk of VCF data lines (`_nodes_found` starts
    empty at every chunk), run here as one device batch.  `-t` is accepted; the chunks' outputs do not depend on it.
    `-S True` (simple selection, find_kmers_over_variant): one batch of per-node searches, no frequency source; -D is not
    consulted, -i / -I are not needed, -N and -H are ignored as in the reference, and -c / -t do not change the output
    (this mode keeps no state from variant to variant).
    Both routes read the VCF through `load_variants` (`--vcf-parse`, `--inflate`)."""
    from .unique_variant_kmers import UniqueVariantKmersFinder, find_kmers_over_variants, load_variant_to_nodes
    if _bool(args.simple):
        if args.vcf is None:
            raise ValueError("make_unique_variant_kmers: -v (the VCF) is required")
        graph = load_graph(args.graph)
        position_id = None if args.position_id_index is None else load_position_id(args.position_id_index, graph)
        flat = find_kmers_over_variants(graph, load_variant_to_nodes(args.variant_to_nodes),
                                        load_variants(args), args.kmer_size, args.max_variant_nodes,
                                        position_id_index=position_id)
        flat.to_file(args.out_file_name)
        logging.info("Wrote %d k-mers (simple selection) to %s" % (len(flat._hashes), args.out_file_name))
        return
    if not _bool(args.use_dense_kmer_finder):
        raise NotImplementedError("make_unique_variant_kmers: only the dense path is supported; pass -D True "
                                  "(the SnpKmerFinder path is not ported)")
    for flag, value in (("-N", args.node_to_variants), ("-H", args.haplotype_matrix)):
        if value is not None:
            raise NotImplementedError("make_unique_variant_kmers: %s is not supported (dense path with a frequency "
                                      "source from -i or -I only)" % flag)
    frequencies = load_frequency_source(args, "make_unique_variant_kmers")
    if args.vcf is None:
        raise ValueError("make_unique_variant_kmers: -v (the VCF) is required")
    graph = load_graph(args.graph)
    finder = UniqueVariantKmersFinder(graph, load_variant_to_nodes(args.variant_to_nodes), load_variants(args),
                                      args.kmer_size, args.max_variant_nodes,
                                      kmer_index_with_frequencies=frequencies,
                                      do_not_choose_lowest_frequency_kmers=_bool(args.do_not_choose_lowest_frequency_kmers),
                                      use_dense_kmer_finder=True,
                                      position_id_index=load_position_id(args.position_id_index, graph),
                                      chunk_size=args.chunk_size)
    flat = finder.find_unique_kmers()
    flat.to_file(args.out_file_name)
    logging.info("Wrote %d k-mers of %d variants to %s" % (len(flat._hashes), finder.last_counts.get("active", 0),
                                                          args.out_file_name))


def sample_kmers_from_structural_variants_command(args):
    """command_line_interface.py:461-481: extra k-mers of big variant nodes, to be merged with the variant k-mers
    (merge_flat_kmers).  `-t` is accepted; all nodes run as one device batch."""
    from .structural_variants import sample_kmers_from_structural_variants
    from .unique_variant_kmers import load_variant_to_nodes
    frequencies = load_frequency_source(args, "sample_kmers_from_structural_variants")
    flat = sample_kmers_from_structural_variants(load_graph(args.graph), load_variant_to_nodes(args.variant_to_nodes),
                                                 frequencies, args.kmer_size)
    flat.to_file(args.out_file_name)
    logging.info("Wrote %d k-mers of structural variant nodes to %s" % (len(flat._hashes), args.out_file_name))


def create_index(args):
    """`make` (command_line_interface.py:105-153) from a linear reference: the reference's chunked output -- 10 * t
    intervals, each ending on the position the next one starts with, each followed by its own reverse complements with
    -r -- as one device call.  The reference's `-t 1` path fails on a linear reference (it adds k to None), so the
    chunked form is used for every -t."""
    from .fasta_files import reference_from_file, resolve_fasta_parse
    from .snp_kmer_finder import make_linear_reference_flat_on_device, read_fasta_record
    if args.graph_file_name is not None:
        raise NotImplementedError("make -g: SnpKmerFinder over a graph is not ported (use `index`); "
                                  "make builds from a linear reference, -R and -n")
    assert args.reference_fasta is not None
    assert args.reference_name is not None, "Reference name must be specified"
    with _lib.DeviceScope() as s:
        if resolve_fasta_parse(args.fasta_parse) == "device":
            letters = s.keep(reference_from_file(args.reference_fasta, [args.reference_name]).letters)
        else:
            letters = read_fasta_record(args.reference_fasta, args.reference_name)
        assert len(letters) > 0, "Length of ref sequennce is 0. Seomthing is wrong"
        flat = s.keep(make_linear_reference_flat_on_device(letters, args.kmer_size, args.spacing, args.genome_size,
                                                           args.threads, _bool(args.include_reverse_complement))).to_flat_kmers()
    logging.info("N kmers in flat kmers: %d" % len(flat._hashes))
    flat.to_file(args.out_file_name)


def make_reference_kmer_index(args):
    """command_line_interface.py:184-193."""
    from .reference_kmer_index import ReferenceKmerIndex
    if args.reference_fasta is not None:
        index = ReferenceKmerIndex.from_linear_reference(args.reference_fasta, args.reference_name, args.kmer_size,
                                                         _bool(args.only_store_kmers), args.fasta_parse)
    else:
        index = ReferenceKmerIndex.from_flat_kmers(FlatKmers.from_file(args.flat_index))
    index.to_file(args.out_file_name)
    logging.info("Saved reference kmer index to file %s" % args.out_file_name)


def merge_flat_kmers(args):
    """command_line_interface.py:489-492."""
    new = FlatKmers.from_multiple_flat_kmers([FlatKmers.from_file(f) for f in args.flat_kmers.split(",")])
    new.to_file(args.out_file_name)
    logging.info("Wrote merged index to %s" % args.out_file_name)


def map_reads_file(args):
    """Reads file -> the node-count vector a genotyper consumes: the role of `kmer_mapper map` next to the reference (its
    flags are not reproduced).  The file is parsed, hashed and probed on the device (read_files.py)."""
    index = CollisionFreeKmerIndex.from_file(args.kmer_index)
    counts = index.map_reads_file(args.reads, args.kmer_size, args.n_nodes, max_hits=args.max_hits,
                                  include_reverse_complement=_bool(args.include_reverse_complement), fmt=args.format,
                                  chunk_bytes=args.chunk_bytes, inflate=args.inflate)
    out = args.out_file_name if args.out_file_name.endswith(".npy") else args.out_file_name + ".npy"
    np.save(out, counts.astype(np.uint32))
    logging.info("Wrote %d node counts (%d hits) to %s" % (len(counts), int(counts.sum(dtype=np.int64)), out))


def make_graph(args):
    """Reference FASTA + VCF -> the graph (GraphArrays.to_file) and its variant-to-nodes table, built on the device
    (graph_files.py).  What it writes is what `-g` and `-V` of the other commands read."""
    from .graph_files import STATUS_TEXT, build_graph_from_files
    chromosomes = None if args.chromosomes is None else [c for c in args.chromosomes.split(",") if c]
    source = None if args.allele_frequencies == "none" else args.allele_frequencies
    built = build_graph_from_files(args.reference_fasta, args.vcf, chromosomes, allele_frequencies=source,
                                   chunk_bytes=args.chunk_bytes, inflate=args.inflate, fasta_parse=args.fasta_parse)
    v2n = args.variant_to_nodes if args.variant_to_nodes is not None else args.out_file_name + ".variant_to_nodes"
    built.graph.to_file(args.out_file_name)
    built.variant_to_nodes.to_file(v2n)
    counts = np.bincount(built.line_status, minlength=len(STATUS_TEXT))
    for code, text in STATUS_TEXT.items():
        logging.info("%d data lines: %s" % (counts[code], text))
    if built.route is not None:
        logging.info("allele frequencies from %s: %d data lines without a value keep 1.0, %d values parsed by the host"
                     % (source, int(np.count_nonzero(built.route == 1)), int(np.count_nonzero(built.route == 2))))
    logging.info("Wrote %d nodes, %d edges and %d bases to %s, variant-to-nodes of %d lines to %s"
                 % (built.graph.n_nodes, len(built.graph.edges), len(built.graph.seq), args.out_file_name,
                    len(built.line_status), v2n))


def make_haplotype_matrix(args):
    """VCF -> the haplotype matrix of its GT columns (HaplotypeMatrix.to_file), parsed on the device (vcf_files.py)."""
    from .vcf_files import DEFAULT_CHUNK_BYTES, haplotype_matrix_from_file
    matrix = haplotype_matrix_from_file(args.vcf, ploidy=args.ploidy, n_samples=args.n_samples,
                                        chunk_bytes=DEFAULT_CHUNK_BYTES if args.chunk_bytes is None else args.chunk_bytes,
                                        inflate=args.inflate)
    matrix.to_file(args.out_file_name, planes=args.planes)
    counts = np.bincount(matrix.codes.reshape(-1), minlength=4)
    logging.info("%d data lines x %d samples of ploidy %d: %d lines hold an unphased GT"
                 % (matrix.n_variants, matrix.n_samples, matrix.ploidy, int(np.count_nonzero(matrix.phased == 0))))
    logging.info("slots: %d allele 0, %d allele 1, %d another allele, %d no allele" % tuple(int(c) for c in counts[:4]))
    logging.info("Wrote the haplotype matrix%s to %s" % (" and its bit planes" if args.planes else "", args.out_file_name))


def open_haplotype_paths(args):
    """The HaplotypePaths of `-g`, `-V` and `-m` (a HaplotypeMatrix file)."""
    from .haplotype_paths import HaplotypePaths
    from .unique_variant_kmers import load_variant_to_nodes
    from .vcf_files import HaplotypeMatrix
    return HaplotypePaths(load_graph(args.graph), load_variant_to_nodes(args.variant_to_nodes),
                          HaplotypeMatrix.from_file(args.haplotype_matrix))


def make_haplotype_to_nodes(args):
    """Graph + variant-to-nodes + haplotype matrix -> the variant nodes every haplotype slot carries
    (HaplotypeToNodes.to_file), listed on the device (haplotype_paths.py)."""
    with open_haplotype_paths(args) as paths:
        table = paths.alt_nodes()
    table.to_file(args.out_file_name)
    logging.info("Wrote %d alt nodes of %d haplotype slots to %s" % (len(table.nodes), table.n_slots, args.out_file_name))


def spell_haplotype(args):
    """One haplotype slot's sequence as a FASTA file with records >1, >2, ... (one per chromosome), lines of 60 letters:
    spelled on the device (haplotype_paths.py), written by the host."""
    from .haplotype_paths import write_fasta
    with open_haplotype_paths(args) as paths, _lib.DeviceScope() as s:
        reference = s.keep(paths.sequence(args.slot))
        write_fasta(args.out_file_name, reference.names, reference.to_host())
        logging.info("Wrote %d letters in %d records of slot %d to %s"
                     % (reference.letters.n, len(reference.names), args.slot, args.out_file_name))


def haplotype_node_counts(args):
    """Node hit counts of the k-mers of some haplotype slots' sequences, one row per slot in the order of `-s`: np.save of
    uint32[slots, nodes] (haplotype_paths.py)."""
    slots = [int(x) for x in args.slots.split(",") if x]
    index = CollisionFreeKmerIndex.from_file(args.kmer_index)
    with open_haplotype_paths(args) as paths:
        route = paths.node_counts_by_difference if args.route == "difference" else paths.node_counts
        counts = route(slots, index, args.kmer_size, args.n_nodes,
                       include_reverse_complement=_bool(args.include_reverse_complement))
    for slot, row in zip(slots, counts):
        logging.info("slot %d: %d hits on %d nodes" % (slot, int(row.sum(dtype=np.int64)), int(np.count_nonzero(row))))
    if args.out_file_name is not None:
        out = args.out_file_name if args.out_file_name.endswith(".npy") else args.out_file_name + ".npy"
        np.save(out, counts)
        logging.info("Wrote the node counts of %d slots to %s" % (len(slots), out))


def make_node_count_model(args):
    """The node count model of some sampled individuals (default: all): per data line, allele and copy number a histogram
    of the allele node's count over the individuals and the counts' sum (NodeCountModel.to_file; haplotype_paths.py)."""
    samples = None if args.samples is None else [int(x) for x in args.samples.split(",") if x]
    index = CollisionFreeKmerIndex.from_file(args.kmer_index)
    with open_haplotype_paths(args) as paths:
        model = paths.node_count_model(index, args.kmer_size, samples, args.n_bins, args.n_nodes,
                                       include_reverse_complement=_bool(args.include_reverse_complement), route=args.route)
    model.to_file(args.out_file_name)
    logging.info("Wrote the node count model of %d individuals over %d data lines (%d bins) to %s"
                 % (len(model.samples), len(model.histogram), model.n_bins, args.out_file_name))


def genotype(args):
    """Genotypes from node counts (what `map` writes) and the node count model, as a VCF: the model fitted once, the rows
    called and the VCF's text made on the device (genotyper.py).  One-dimensional counts are one sample and one sample
    column; two-dimensional counts, or a comma-separated list of one-dimensional files, are a cohort: one VCF with a column
    per row, the rows called in batches of at most --batch-bytes of counts."""
    from .genotyper import Genotyper, write_genotyped_vcf
    from .haplotype_paths import NodeCountModel
    from .unique_variant_kmers import load_variant_to_nodes
    if "," in args.counts:
        rows = [np.load(name) for name in args.counts.split(",")]
        if any(r.ndim != 1 for r in rows) or len({len(r) for r in rows}) != 1:
            raise ValueError("%s: a list of counts files holds one-dimensional rows of one length" % args.counts)
        counts = np.stack(rows)
    else:
        counts = np.load(args.counts)
    if counts.ndim == 2:
        return genotype_cohort(args, counts)
    if counts.ndim != 1:
        raise ValueError("%s holds %d-dimensional counts: genotype takes one sample's row or a batch of rows"
                         % (args.counts, counts.ndim))
    if isinstance(args.coverage, tuple):
        raise ValueError("--coverage takes one number for one sample's row")
    with Genotyper(NodeCountModel.from_file(args.model), load_variant_to_nodes(args.variant_to_nodes), args.error,
                   args.pseudo_count) as genotyper:
        ploidy = genotyper.ploidy
        calls = genotyper.genotype(counts, args.coverage, loglik=args.loglik is not None)
    if args.loglik is not None:
        np.save(args.loglik if args.loglik.endswith(".npy") else args.loglik + ".npy", calls.loglik)
    n = write_genotyped_vcf(args.vcf, args.out_file_name, calls.call, calls.gq, ploidy, args.sample_name, args.chunk_bytes,
                            args.inflate, compress=output_compression(args.compress, args.out_file_name))
    logging.info("Wrote %d data lines (%d not called) at coverage %g to %s"
                 % (n, int(np.count_nonzero(calls.call < 0)), calls.coverage[0], args.out_file_name))


def genotype_cohort(args, counts):
    """`genotype` for counts uint32[S][n_nodes]: every row called with the one fitted model, in batches whose counts hold at
    most --batch-bytes (a row's calls do not depend on its batch), and one VCF with S sample columns written."""
    from .genotyper import Genotyper, check_sample_names, write_cohort_vcf
    from .haplotype_paths import NodeCountModel
    from .unique_variant_kmers import load_variant_to_nodes
    n_samples, n_nodes = counts.shape
    if n_samples < 1:
        raise ValueError("%s holds no row" % args.counts)
    if n_samples > 1 and args.sample_name == "sample":     # the option's default
        names = ["sample_%d" % (i + 1) for i in range(n_samples)]
    else:
        names = check_sample_names(args.sample_name.split(","))
    if len(names) != n_samples:
        raise ValueError("%d sample names for %d rows of counts" % (len(names), n_samples))
    coverage = None
    if args.coverage is not None:
        coverage = np.array(args.coverage if isinstance(args.coverage, tuple) else [args.coverage], dtype=np.float64)
        if len(coverage) not in (1, n_samples):
            raise ValueError("--coverage takes one number or one per row: %d for %d rows" % (len(coverage), n_samples))
        coverage = np.ascontiguousarray(np.broadcast_to(coverage, (n_samples,)))
    if args.batch_bytes < 1:
        raise ValueError("--batch-bytes must be positive")
    rows_per_batch = int(min(65535, max(1, args.batch_bytes // max(4 * n_nodes, 1))))
    parts = []
    with Genotyper(NodeCountModel.from_file(args.model), load_variant_to_nodes(args.variant_to_nodes), args.error,
                   args.pseudo_count) as genotyper:
        ploidy = genotyper.ploidy
        for at in range(0, n_samples, rows_per_batch):
            to = min(n_samples, at + rows_per_batch)
            parts.append(genotyper.genotype(counts[at:to], None if coverage is None else coverage[at:to],
                                            loglik=args.loglik is not None))
    call, gq = np.concatenate([p.call for p in parts]), np.concatenate([p.gq for p in parts])
    if args.loglik is not None:
        np.save(args.loglik if args.loglik.endswith(".npy") else args.loglik + ".npy", np.concatenate([p.loglik for p in parts]))
    n = write_cohort_vcf(args.vcf, args.out_file_name, call, gq, ploidy, names, args.chunk_bytes, args.inflate,
                         compress=output_compression(args.compress, args.out_file_name))
    lam = np.concatenate([p.coverage for p in parts])
    logging.info("Wrote %d data lines with %d sample columns (%d calls not made) at coverages %g .. %g to %s"
                 % (n, n_samples, int(np.count_nonzero(call < 0)), lam.min(), lam.max(), args.out_file_name))


def _coverage(text):
    """`--coverage`: one number as a float, comma-separated numbers as a tuple of floats."""
    values = tuple(float(x) for x in text.split(","))
    return values[0] if len(values) == 1 else values


def output_compression(compress, out_file_name):
    """`--compress`: none and bgzf are themselves, auto is bgzf for a name that ends in .gz."""
    if compress == "auto":
        return "bgzf" if str(out_file_name).endswith(".gz") else "none"
    return compress


def bgzf_command(args):
    """A plain file -> a BGZF file deflated on the device (bgzf.write_bgzf_on_device): the conversion the `--inflate device`
    routes ask for, without a host `bgzip` run."""
    from .bgzf import write_bgzf_on_device
    n = write_bgzf_on_device(args.out_file_name, args.in_file_name, args.block_size, args.chunk_bytes)
    logging.info("Wrote %d bytes of BGZF to %s" % (n, args.out_file_name))


def _haplotype_paths_arguments(p):
    p.add_argument("-g", "--graph", required=True)
    p.add_argument("-V", "--variant_to_nodes", required=True, help="built with the graph (make_graph writes both)")
    p.add_argument("-m", "--haplotype-matrix", required=True, help="what make_haplotype_matrix writes, from the same VCF")


def build_parser():
    parser = argparse.ArgumentParser(description="graph_kmer_index on MI355X (in-scope sub-commands)")
    sub = parser.add_subparsers()
    p = sub.add_parser("index")
    p.add_argument("-g", "--graph", required=True)
    p.add_argument("-c", "--critical_graph_paths", required=False)
    p.add_argument("-p", "--position_id", required=False)
    p.add_argument("-k", "--kmer-size", type=int, default=31)
    p.add_argument("-o", "--out-file-name", required=True)
    p.add_argument("-t", "--n-threads", type=int, default=1)
    p.add_argument("-w", "--whitelist", required=False)
    p.add_argument("-r", "--include-reverse-complement", type=_bool, default=False)
    p.add_argument("-O", "--only-save-one-node-per-kmer", type=_bool, default=False)
    p.add_argument("-v", "--max-variant-nodes", type=int, default=5)
    p.add_argument("--ranks", type=int, default=0, help="processes of `-t N` (default: min(N, visible devices); more ranks "
                   "than devices share them round-robin)")
    p.add_argument("--shard", default=None, help=argparse.SUPPRESS)       # R/W: this process is rank R of `index -t`
    p.set_defaults(func=index)
    p = sub.add_parser("make")
    p.add_argument("-g", "--graph_file_name", required=False)
    p.add_argument("-o", "--out_file_name", required=True)
    p.add_argument("-k", "--kmer_size", required=False, type=int, default=31)
    p.add_argument("-r", "--include-reverse-complement", required=False, type=_bool, default=False)
    p.add_argument("-s", "--spacing", required=False, type=int, default=31)
    p.add_argument("-p", "--pruning", required=False, type=_bool, default=False)
    p.add_argument("-m", "--max-kmers-same-position", required=False, type=int, default=100000)
    p.add_argument("-M", "--max-frequency", required=False, type=int, default=10000000)
    p.add_argument("-v", "--max-variant-nodes", required=False, type=int, default=100000)
    p.add_argument("-V", "--only-add-variant-kmers", required=False, type=_bool, default=False)
    p.add_argument("-N", "--only-save-variant-nodes", required=False, type=_bool, default=False)
    p.add_argument("-O", "--only-save-one-node-per-kmer", required=False, type=_bool, default=False)
    p.add_argument("-S", "--skip-kmers-with-nodes", required=False)
    p.add_argument("-w", "--whitelist", required=False)
    p.add_argument("-t", "--threads", required=False, default=1, type=int)
    p.add_argument("-G", "--genome-size", required=False, default=3000000000, type=int)
    p.add_argument("-R", "--reference-fasta", required=False)
    p.add_argument("-n", "--reference-name", required=False)
    p.add_argument("--fasta-parse", required=False, choices=("auto", "host", "device"), default="auto",
                   help="where the reference FASTA (.fa, or .fa.gz as BGZF or gzip) is parsed: auto = device; host = on "
                        "the host with NumPy")
    p.set_defaults(func=create_index)
    p = sub.add_parser("make_reference_kmer_index")
    p.add_argument("-f", "--flat-index", required=False)
    p.add_argument("-r", "--reference-fasta", required=False)
    p.add_argument("-n", "--reference-name", required=False)
    p.add_argument("-k", "--kmer-size", required=False, type=int, default=16)
    p.add_argument("-o", "--out-file-name", required=True)
    p.add_argument("-O", "--only-store-kmers", required=False, default=False, type=_bool)
    p.add_argument("--fasta-parse", required=False, choices=("auto", "host", "device"), default="auto",
                   help="where the reference FASTA (.fa, or .fa.gz as BGZF or gzip) is parsed: auto = device; host = on "
                        "the host with NumPy")
    p.set_defaults(func=make_reference_kmer_index)
    p = sub.add_parser("merge_flat_kmers")
    p.add_argument("-f", "--flat-kmers", required=True)
    p.add_argument("-o", "--out-file-name", required=True)
    p.set_defaults(func=merge_flat_kmers)
    p = sub.add_parser("make_from_flat")
    p.add_argument("-o", "--out_file_name", required=True)
    p.add_argument("-f", "--flat-index", required=True)
    p.add_argument("-m", "--hash_modulo", type=int, default=452930477)
    p.add_argument("-S", "--skip-frequencies", type=_bool, default=False)
    p.add_argument("-M", "--make-minimal", type=_bool, default=False)
    p.add_argument("-r", "--add-reverse-complements", type=_bool, default=False)
    p.add_argument("-k", "--kmer-size", type=int, default=31)
    p.add_argument("-s", "--skip-singletons", type=_bool, default=False)
    p.set_defaults(func=make_from_flat)
    p = sub.add_parser("find_critical_paths")
    p.add_argument("-g", "--graph", required=True)
    p.add_argument("-k", "--kmer-size", type=int, default=31)
    p.add_argument("-o", "--out-file-name", required=True)
    p.set_defaults(func=find_critical_paths)
    p = sub.add_parser("add_reverse_complements")
    p.add_argument("-f", "--flat-kmers", required=True)
    p.add_argument("-o", "--out-file-name", required=True)
    p.add_argument("-k", "--kmer-size", type=int, required=True)
    p.set_defaults(func=add_reverse_complements)
    p = sub.add_parser("make_reverse")
    p.add_argument("-f", "--flat-index", required=True)
    p.add_argument("-o", "--out-file-name", required=True)
    p.set_defaults(func=make_reverse)
    p = sub.add_parser("make_unique_variant_kmers")
    p.add_argument("-g", "--graph", required=True)
    p.add_argument("-V", "--variant_to_nodes", required=True)
    p.add_argument("-N", "--node-to-variants", required=False)
    p.add_argument("-H", "--haplotype-matrix", required=False)
    p.add_argument("-k", "--kmer-size", required=True, type=int)
    p.add_argument("-i", "--kmer-index", required=False)
    p.add_argument("-I", "--kmer-counter", required=False)
    p.add_argument("-p", "--position-id-index", required=False)
    p.add_argument("-D", "--use-dense-kmer-finder", required=False, type=_bool, default=False)
    p.add_argument("-o", "--out-file-name", required=True)
    p.add_argument("-v", "--vcf", required=False)
    p.add_argument("-t", "--n-threads", required=False, default=1, type=int)
    p.add_argument("-c", "--chunk-size", required=False, default=10000, type=int)
    p.add_argument("-m", "--max-variant-nodes", required=False, default=6, type=int)
    p.add_argument("-d", "--do-not-choose-lowest-frequency-kmers", required=False, type=_bool, default=False)
    p.add_argument("-S", "--simple", type=_bool, default=False)
    p.add_argument("--vcf-parse", required=False, choices=("auto", "host", "device"), default="auto",
                   help="where the VCF's lines are parsed: auto = device; host = line by line in Python")
    p.add_argument("--inflate", required=False, choices=("auto", "host", "device"), default="auto",
                   help="where a .gz VCF is inflated when it is parsed on the device: auto = BGZF on the device, other gzip "
                        "on the host; device refuses a file that is not BGZF")
    p.set_defaults(func=make_unique_variant_kmers)
    p = sub.add_parser("sample_kmers_from_structural_variants")
    p.add_argument("-g", "--graph", required=True)
    p.add_argument("-V", "--variant_to_nodes", required=True)
    p.add_argument("-k", "--kmer-size", required=True, type=int)
    p.add_argument("-i", "--kmer-index", required=False)
    p.add_argument("-I", "--kmer-counter", required=False)
    p.add_argument("-o", "--out-file-name", required=True)
    p.add_argument("-t", "--n-threads", required=False, default=1, type=int)
    p.set_defaults(func=sample_kmers_from_structural_variants_command)
    p = sub.add_parser("count_kmers")
    p.add_argument("-f", "--flat-kmers", required=True)
    p.add_argument("-o", "--out-file-name", required=True)
    p.add_argument("-m", "--modulo", required=False, type=int, default=0)
    p.add_argument("-s", "--subsample-ratio", required=False, type=int, default=1,
                   help="1 to keep every kmer, 2 for every other etc")
    p.set_defaults(func=count_kmers)
    p = sub.add_parser("make_kmer_frequency_index")
    p.add_argument("-r", "--reference-kmers", required=True)
    p.add_argument("-o", "--out-file-name", required=True)
    p.set_defaults(func=make_kmer_frequencies)
    p = sub.add_parser("make_graph")
    p.add_argument("-r", "--reference-fasta", required=True)
    p.add_argument("-v", "--vcf", required=True, help="VCF, optionally .gz (BGZF or gzip)")
    p.add_argument("-o", "--out-file-name", required=True, help="the graph, as GraphArrays.to_file writes it")
    p.add_argument("-n", "--chromosomes", required=False, default=None,
                   help="comma-separated FASTA record names in graph order (default: every record, in file order)")
    p.add_argument("-V", "--variant-to-nodes", required=False, default=None, help="default: <out>.variant_to_nodes")
    p.add_argument("-a", "--allele-frequencies", required=False, choices=("none", "info", "genotypes"), default="none",
                   help="where the allele nodes' frequencies come from: none = 1.0 on every node; info = the AF= entry of "
                        "INFO; genotypes = the GT columns, counted on the device.  A line without a value keeps 1.0")
    p.add_argument("--inflate", required=False, choices=("auto", "host", "device"), default="auto",
                   help="where a .gz VCF is inflated: auto = BGZF on the device, other gzip on the host")
    p.add_argument("--chunk-bytes", required=False, type=int, default=None)
    p.add_argument("--fasta-parse", required=False, choices=("auto", "host", "device"), default="auto",
                   help="where the reference FASTA (.fa, or .fa.gz as BGZF or gzip) is parsed: auto = device; host = on "
                        "the host with NumPy")
    p.set_defaults(func=make_graph)
    p = sub.add_parser("make_haplotype_matrix")
    p.add_argument("-v", "--vcf", required=True, help="VCF with GT columns, optionally .gz (BGZF or gzip)")
    p.add_argument("-o", "--out-file-name", required=True, help="the matrix, as HaplotypeMatrix.to_file writes it (.npz)")
    p.add_argument("-p", "--ploidy", required=False, type=int, default=2, help="slots per sample, 1 to 8")
    p.add_argument("-s", "--n-samples", required=False, type=int, default=None,
                   help="default: the sample columns of the #CHROM header line, else of the first data line")
    p.add_argument("--planes", required=False, type=_bool, default=False,
                   help="also write ref_bits and alt_bits, one bit per slot and line")
    p.add_argument("--inflate", required=False, choices=("auto", "host", "device"), default="auto",
                   help="where a .gz VCF is inflated: auto = BGZF on the device, other gzip on the host")
    p.add_argument("--chunk-bytes", required=False, type=int, default=None)
    p.set_defaults(func=make_haplotype_matrix)
    p = sub.add_parser("make_haplotype_to_nodes")
    _haplotype_paths_arguments(p)
    p.add_argument("-o", "--out-file-name", required=True, help="the table, as HaplotypeToNodes.to_file writes it (.npz)")
    p.set_defaults(func=make_haplotype_to_nodes)
    p = sub.add_parser("spell_haplotype")
    _haplotype_paths_arguments(p)
    p.add_argument("-s", "--slot", required=True, type=int, help="sample * ploidy + haplotype of the sample")
    p.add_argument("-o", "--out-file-name", required=True, help="FASTA, a record per chromosome named 1, 2, ...")
    p.set_defaults(func=spell_haplotype)
    p = sub.add_parser("haplotype_node_counts")
    _haplotype_paths_arguments(p)
    p.add_argument("-i", "--kmer-index", required=True)
    p.add_argument("-k", "--kmer-size", required=False, type=int, default=31)
    p.add_argument("-s", "--slots", required=True, help="comma-separated haplotype slots, a row of counts each")
    p.add_argument("-o", "--out-file-name", required=False, default=None, help="np.save of uint32[slots, nodes]")
    p.add_argument("-n", "--n-nodes", required=False, type=int, default=None, help="default: the index's max node id + 1")
    p.add_argument("-r", "--include-reverse-complement", required=False, type=_bool, default=True)
    p.add_argument("--route", required=False, choices=("whole", "difference"), default="whole",
                   help="whole: hash and probe every k-mer of a slot; difference: only those that differ from the all-ref path")
    p.set_defaults(func=haplotype_node_counts)
    p = sub.add_parser("make_node_count_model")
    _haplotype_paths_arguments(p)
    p.add_argument("-i", "--kmer-index", required=True)
    p.add_argument("-k", "--kmer-size", required=False, type=int, default=31)
    p.add_argument("-s", "--samples", required=False, default=None, help="comma-separated individuals; default: all")
    p.add_argument("-b", "--n-bins", required=False, type=int, default=5, help="counts of n_bins - 1 and more share the last bin")
    p.add_argument("-n", "--n-nodes", required=False, type=int, default=None, help="default: the index's max node id + 1")
    p.add_argument("-r", "--include-reverse-complement", required=False, type=_bool, default=True)
    p.add_argument("--route", required=False, choices=("whole", "difference"), default="difference")
    p.add_argument("-o", "--out-file-name", required=True, help="the model, as NodeCountModel.to_file writes it (.npz)")
    p.set_defaults(func=make_node_count_model)
    p = sub.add_parser("genotype")
    p.add_argument("-V", "--variant_to_nodes", required=True, help="built with the graph (make_graph writes both)")
    p.add_argument("-M", "--model", required=True, help="what make_node_count_model writes")
    p.add_argument("-c", "--counts", required=True,
                   help="node counts as map writes them (.npy): one sample's row; or a cohort, as a two-dimensional .npy "
                        "or a comma-separated list of one-dimensional files, for one VCF with a column per row")
    p.add_argument("-v", "--vcf", required=True, help="the VCF the graph was made from, optionally .gz (BGZF or gzip)")
    p.add_argument("-o", "--out-file-name", required=True, help="the genotyped VCF: plain text, or BGZF as --compress says")
    p.add_argument("-s", "--sample-name", required=False, default="sample",
                   help="the sample's name, for a cohort comma-separated names; the default is sample_1 .. sample_S for a "
                        "cohort of more than one row")
    p.add_argument("--coverage", required=False, type=_coverage, default=None,
                   help="the sample's coverage relative to the model's individuals, for a cohort one number or one per row, "
                        "comma-separated; default: estimated from the counts")
    p.add_argument("--batch-bytes", required=False, type=int, default=1 << 30,
                   help="a cohort's rows are called in batches whose counts hold at most this many bytes")
    p.add_argument("--error", required=False, type=float, default=0.01)
    p.add_argument("--pseudo-count", required=False, type=float, default=1.0)
    p.add_argument("-L", "--loglik", required=False, default=None, help="np.save of float64[lines, ploidy + 1], for a cohort [rows, lines, ploidy + 1]")
    p.add_argument("--inflate", required=False, choices=("auto", "host", "device"), default="auto",
                   help="where a .gz VCF is inflated: auto = BGZF on the device, other gzip on the host")
    p.add_argument("--chunk-bytes", required=False, type=int, default=None)
    p.add_argument("--compress", required=False, choices=("none", "bgzf", "auto"), default="none",
                   help="bgzf = the VCF leaves as BGZF, deflated on the device; auto = bgzf when -o ends in .gz")
    p.set_defaults(func=genotype)
    p = sub.add_parser("bgzf")
    p.add_argument("-i", "--in-file-name", required=True, help="a plain file: FASTA, FASTQ, VCF, any text")
    p.add_argument("-o", "--out-file-name", required=True, help="the BGZF file (.gz)")
    p.add_argument("--block-size", required=False, type=int, default=0xff00, help="input bytes per member, 1..65280")
    p.add_argument("--chunk-bytes", required=False, type=int, default=64 << 20, help="bytes per read of the input")
    p.set_defaults(func=bgzf_command)
    p = sub.add_parser("map")
    p.add_argument("-i", "--kmer-index", required=True)
    p.add_argument("-f", "--reads", required=True, help="FASTA or FASTQ, optionally .gz (gzip or BGZF)")
    p.add_argument("-k", "--kmer-size", required=False, type=int, default=31)
    p.add_argument("-o", "--out-file-name", required=True, help="np.save of the uint32 node counts")
    p.add_argument("-n", "--n-nodes", required=False, type=int, default=None, help="default: the index's max node id + 1")
    p.add_argument("-r", "--include-reverse-complement", required=False, type=_bool, default=True)
    p.add_argument("-m", "--max-hits", required=False, type=int, default=2 ** 62)
    p.add_argument("-c", "--chunk-bytes", required=False, type=int, default=None)
    p.add_argument("-F", "--format", required=False, choices=("fasta", "fastq"), default=None,
                   help="default: by the file's first byte")
    p.add_argument("--inflate", required=False, choices=("auto", "host", "device"), default="auto",
                   help="where a .gz file is inflated: auto = BGZF on the device, other gzip on the host; device refuses a "
                        "file that is not BGZF")
    p.add_argument("-t", "--n-threads", required=False, default=1, type=int)
    p.set_defaults(func=map_reads_file)
    return parser


def main(argv=None):
    logging.basicConfig(level=logging.INFO)
    parser = build_parser()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    if not hasattr(args, "func"):
        parser.print_help()
        return 1
    args.func(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
