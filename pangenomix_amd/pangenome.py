"""
Pan-genome construction on MI355X: host side of the hot path.

Drop-in mirror of the reference entry points in pangenomix/pangenome.py
(file:line cited per function) for the path SURVEY.md §8 scopes:

  build_cds_pangenome / build_noncoding_pangenome
     consolidate_seqs              exact dedupe by sha256          (H1)
   * cluster_with_cdhit            greedy clustering -> HIP (K1/K2) instead of
                                   the `cd-hit` / `cd-hit-est` shell-out
     rename_genes_and_alleles      .clstr -> <name>_C#A# names      (H2)
     build_genetic_feature_tables  allele x genome, gene x genome   (H4)
     LightSparseDataFrame.to_npz   .npz + .labels.txt               (H5)
     extract_noncoding             GFF+FNA -> feature FASTA         (H6)
  build_upstream/downstream/proximal_pangenome   5'/3' UTR pangenomes
  validate_upstream/downstream/proximal_table_direct   the recorded UTRs searched in the genomes -> HIP (csrc/scan.hip)
  validate_table_against_fasta, validate_allele/upstream/downstream_table   every FASTA record looked up among the
                                   non-redundant sequences -> HIP (csrc/dict.hip)

Same names, positional order, defaults, intermediate files and return values.
The only behavioural differences are deliberate: a failing
clustering call raises instead of surfacing later as FileNotFoundError, and
unknown `cdhit_args` keys are rejected instead of silently passed through.
"""

from __future__ import print_function
import collections
import os
import hashlib
import shutil
import subprocess as sp
import urllib.parse

import numpy as np
import scipy.sparse

from . import sparse_utils

LOG_RATE = 10  # reference pangenome.py:32
CLUSTER_TYPES = {'cds': 'C', 'noncoding': 'T'}
VARIANT_TYPES = {'allele': 'A', 'upstream': 'U', 'downstream': 'D'}
_COMPLEMENT = str.maketrans('ACGTWSRYMKNacgtwsrymkn', 'TGCAWSYRKMNtgcawsyrkmn')
_COMPLEMENT_KEYS = frozenset('ACGTWSRYMKNacgtwsrymkn')


# ---------------------------------------------------------------------------
# small helpers (reference pangenome.py:1938-1969, :2040-2059)
# ---------------------------------------------------------------------------
def __get_gene_from_allele__(allele):
    """<name>_C#A# -> <name>_C# (reference :2040-2044: split on the last 'A')."""
    return allele[:allele.rindex('A')] if 'A' in allele else ''


def __get_genome_from_filename__(filepath):
    """Basename without extension (reference :2046-2051)."""
    return os.path.splitext(os.path.split(filepath)[1])[0]


def __get_header_from_fasta_line__(line):
    """First whitespace token minus '>' (reference :2053-2055)."""
    return line.split()[0][1:].strip()


def __hash_sequence__(seq):
    return hashlib.sha256(seq.encode('utf-8')).digest()


def reverse_complement(seq):
    """Reference :1938-1941 (table :37-41); unknown bases raise KeyError there."""
    for base in seq:
        if base not in _COMPLEMENT_KEYS:
            raise KeyError(base)
    return seq.translate(_COMPLEMENT)[::-1]


def create_feature_name(name, cluster_type, cluster_num, variant_type=None, variant_num=-1):
    """<name>_<C|T><cluster>[<A|U|D><variant>] (reference :1944-1969)."""
    short = name + '_' + CLUSTER_TYPES[cluster_type] + str(cluster_num)
    if variant_type is not None and int(variant_num) >= 0:
        short += VARIANT_TYPES[variant_type] + str(variant_num)
    return short


def list_faa_files(directory_path):
    """*.faa in os.listdir order, unsorted (reference :407-423)."""
    return [os.path.join(directory_path, f) for f in os.listdir(directory_path)
            if f.endswith('.faa')]


def find_matching_genome_files(gff_dir, fna_dir):
    """(gff, fna) pairs sharing a basename, in FNA listing order (reference :318-334)."""
    gff = {os.path.splitext(f)[0]: os.path.join(gff_dir, f)
           for f in os.listdir(gff_dir) if f.endswith('.gff')}
    pairs = []
    for f in os.listdir(fna_dir):
        if f.endswith('.fna') and os.path.splitext(f)[0] in gff:
            pairs.append((gff[os.path.splitext(f)[0]], os.path.join(fna_dir, f)))
    return pairs


def _iter_fasta_records(path):
    """Yields (header_token, [stripped sequence lines]) as the reference's line
    scanners see them (:381-391, :638-656): a record starts at a line whose first
    character is '>', sequence lines are .strip()-ed, lines before the first
    header belong to an empty header."""
    header, blocks = '', []
    with open(path, 'r') as f:
        for line in f:
            if line[0] == '>':
                yield header, blocks
                header, blocks = __get_header_from_fasta_line__(line), []
            else:
                blocks.append(line.strip())
    yield header, blocks


def load_sequences_from_fasta(fasta, header_fxn=None, seq_fxn=None, filter_fxn=None):
    """Header -> sequence dict (reference :1892-1916); full header line by default."""
    out = {}
    header, blocks = '', []

    def flush():
        seq = ''.join(blocks)
        if header and seq and (filter_fxn is None or filter_fxn(header)):
            out[header] = seq_fxn(seq) if seq_fxn else seq
    with open(fasta, 'r') as f:
        for line in f:
            if line[0] == '>':
                flush()
                header = line.strip()[1:]
                header = header_fxn(header) if header_fxn else header
                blocks = []
            else:
                blocks.append(line.strip())
    flush()
    return out


# ---------------------------------------------------------------------------
# H1: exact-duplicate consolidation (reference :336-405)
# ---------------------------------------------------------------------------
def consolidate_seqs(genome_paths, nr_out, shared_headers_out, missing_headers_out=None):
    """Merge genome FASTA files into one non-redundant FASTA.

    Files are read in the order given; the first header seen for a sequence is
    its representative and the record is written with its original line
    wrapping. Returns ({sha256 digest: [headers]}, [headers without sequence]).
    """
    groups = {}     # digest -> headers in order observed (insertion order = encounter order)
    missing = []
    with open(nr_out, 'w+') as f_nr:
        for path in genome_paths:
            for header, blocks in _iter_fasta_records(path):
                if not header:
                    continue
                seq = ''.join(blocks)
                if not seq:
                    missing.append(header)
                    continue
                digest = __hash_sequence__(seq)
                known = groups.get(digest)
                if known is None:
                    groups[digest] = [header]
                    f_nr.write('>' + header + '\n' + '\n'.join(blocks) + '\n')
                else:
                    known.append(header)
    with open(shared_headers_out, 'w+') as f:
        for headers in groups.values():
            if len(headers) > 1:
                f.write('\t'.join(headers) + '\n')
    if missing_headers_out:
        print('Headers without sequences:', len(missing))
        with open(missing_headers_out, 'w+') as f:
            for header in missing:
                f.write(header + '\n')
    return groups, missing


# ---------------------------------------------------------------------------
# K1/K2: greedy incremental clustering on the GPU
# ---------------------------------------------------------------------------
def cluster_with_cdhit(fasta_file, cdhit_out, cdhit_args={'-n': 5, '-c': 0.8}):
    """Cluster a FASTA file; writes `cdhit_out` (representatives) and
    `cdhit_out + '.clstr'` exactly where the reference's cd-hit call would
    (reference :425-450). `.fna` input selects the nucleotide (cd-hit-est) rules.

    The clustering itself runs in the HIP library (pangenomix_amd.cluster);
    there is no CPU fallback: a missing library or GPU raises.
    """
    from . import cluster
    cluster.cluster_fasta_to_clstr(fasta_file, cdhit_out, cdhit_args)


# ---------------------------------------------------------------------------
# H2: .clstr -> allele names (reference :453-560)
# ---------------------------------------------------------------------------
def _parse_clstr(clstr_file):
    """Yields (cluster_num_str, member_num_str, header) per member line, using
    exactly the tokens the reference consumes (:505-513, :716-724)."""
    cluster_num = None
    with open(clstr_file, 'r') as f:
        for line in f:
            if line[0] == '>':
                cluster_num = line.split()[-1].strip()
            else:
                data = line.split()
                yield cluster_num, data[0], data[2][1:-3]


def rename_genes_and_alleles(clstr_file, nr_fasta_in, nr_fasta_out,
                             feature_names_out, name='Test', cluster_type='cds',
                             shared_headers_file=None, fastasort_path=None):
    """Name every clustered sequence <name>_C#A# / <name>_T#A#, write the
    name table, and rewrite the non-redundant FASTA with the new headers.
    Returns {original header (incl. synonyms): allele name}."""
    synonyms = {}
    if shared_headers_file:
        with open(shared_headers_file, 'r') as f:
            for line in f:
                headers = line.strip().split('\t')
                synonyms[headers[0]] = headers[1:]

    header_to_allele = {}
    with open(feature_names_out, 'w+') as f_names:
        for cluster_num, member_num, header in _parse_clstr(clstr_file):
            allele = create_feature_name(name, cluster_type, cluster_num, 'allele', member_num)
            header_to_allele[header] = allele
            mapped = [header]
            for syn in synonyms.get(header, ()):
                header_to_allele[syn] = allele
                mapped.append(syn)
            f_names.write(allele + '\t' + '\t'.join(mapped).strip() + '\n')

    tmp = nr_fasta_out + '.tmp'
    with open(nr_fasta_in, 'r') as f_old, open(tmp, 'w+') as f_new:
        keep = False
        for line in f_old:
            if line[0] == '>':
                header = line[1:].strip()
                allele = header_to_allele.get(header)
                keep = allele is not None
                if keep:
                    f_new.write('>' + allele + '\n')
                else:
                    print('MISSING:', header)
            elif keep:
                f_new.write(line)
    if nr_fasta_out == nr_fasta_in:
        os.remove(nr_fasta_in)
    os.rename(tmp, nr_fasta_out)

    if fastasort_path:  # optional external Exonerate fastasort (reference :547-559)
        print('Sorting sequences by header...')
        with open(tmp, 'w+') as f_sort:
            p = sp.Popen(['./' + fastasort_path, nr_fasta_out], stdout=f_sort, stderr=sp.PIPE)
            _, stderr = p.communicate()
            print(stderr)
        if p.returncode == 1:
            print('Aborting sort, exitcode', p.returncode)
            os.remove(tmp)
        else:
            os.rename(tmp, nr_fasta_out)
    return header_to_allele


# ---------------------------------------------------------------------------
# H3: header -> allele map (reference :683-740)
# ---------------------------------------------------------------------------
def load_header_to_allele(clstr_file=None, shared_header_file=None,
                          header_to_allele=None, name='Test', cluster_type='cds'):
    if header_to_allele is None:
        full = {}
        for cluster_num, member_num, header in _parse_clstr(clstr_file):
            full[header] = create_feature_name(name, cluster_type, cluster_num, 'allele', member_num)
    else:
        full = dict(header_to_allele)
    if shared_header_file:
        with open(shared_header_file, 'r') as f:
            for line in f:
                headers = [x.strip() for x in line.split('\t')]
                for alt in headers[1:]:
                    full[alt] = full[headers[0]]
    return full


# ---------------------------------------------------------------------------
# H4: allele x genome and gene x genome tables (reference :563-680)
# ---------------------------------------------------------------------------
def _first_occurrence_coo(rows, cols, n_rows, n_cols):
    """COO with ones, duplicates dropped, triples in order of first insertion:
    the order scipy's dok_matrix.tocoo() yields for the reference's loop
    (:649-650), pinned by tests/golden/cds."""
    from . import _native
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    first = _native.first_insertions(rows, cols, n_cols)            # hash-based: linear, keeps the order
    data = np.ones(first.size, dtype=np.int64)
    return scipy.sparse.coo_matrix(
        (data, (rows[first].astype(np.int32), cols[first].astype(np.int32))),
        shape=(n_rows, n_cols))


def build_genetic_feature_tables(clstr_file, genome_fasta_paths, name='Test', cluster_type='cds',
                                 output_format='lsdf', shared_header_file=None,
                                 header_to_allele=None, log_rate=LOG_RATE):
    """Binary allele x genome and gene x genome tables as LSDFs.

    Row labels are the lexicographically sorted allele names (so C100 < C10 <
    C11 < C1 < C2, reference :615) and their consecutive-deduped gene prefixes
    (:618-623); columns are the sorted genome basenames (:612). Genome files are
    scanned in sorted(path) order (:635) and a record counts only if it has a
    non-empty sequence (:643).
    """
    print('Loadings header-allele mappings...')
    # NB the reference passes cluster_type into the `name` slot here (:608-609);
    # harmless because the dict is always supplied on the hot path.
    header_to_allele = load_header_to_allele(clstr_file, shared_header_file,
                                             header_to_allele, cluster_type)
    genome_order = sorted(__get_genome_from_filename__(p) for p in genome_fasta_paths)
    print('Sorting alleles...')
    allele_order = sorted(set(header_to_allele.values()))
    print('Sorting clusters...')
    gene_of_allele = np.empty(len(allele_order), dtype=np.int64)
    gene_order, last = [], None
    for i, allele in enumerate(allele_order):
        gene = __get_gene_from_allele__(allele)
        if gene != last:
            gene_order.append(gene)
            last = gene
        gene_of_allele[i] = len(gene_order) - 1
    print('Genomes:', len(genome_order))
    print('Clusters:', len(gene_order))
    print('Alleles:', len(allele_order))

    allele_index = {a: i for i, a in enumerate(allele_order)}
    header_index = {h: allele_index[a] for h, a in header_to_allele.items()}
    genome_index = {}
    for i, g in enumerate(genome_order):
        genome_index.setdefault(g, i)      # list.index() semantics: first match

    rec_allele, rec_genome = [], []
    for i, path in enumerate(sorted(genome_fasta_paths)):
        genome = __get_genome_from_filename__(path)
        genome_i = genome_index[genome]
        for header, blocks in _iter_fasta_records(path):
            if not any(blocks):
                continue
            allele_i = header_index.get(header)
            if allele_i is None:
                print('MISSING:', header)
                continue
            rec_allele.append(allele_i)
            rec_genome.append(genome_i)
        if (i + 1) % log_rate == 0:
            print('Updating genome', i + 1, ':', genome)

    print('Building binary matrix...')
    rec_allele = np.asarray(rec_allele, dtype=np.int64)
    rec_genome = np.asarray(rec_genome, dtype=np.int64)
    sp_alleles = _first_occurrence_coo(rec_allele, rec_genome, len(allele_order), len(genome_order))
    sp_genes = _first_occurrence_coo(gene_of_allele[rec_allele] if rec_allele.size else rec_allele,
                                     rec_genome, len(gene_order), len(genome_order))
    df_alleles = sparse_utils.LightSparseDataFrame(allele_order, genome_order, sp_alleles)
    df_genes = sparse_utils.LightSparseDataFrame(gene_order, genome_order, sp_genes)
    if output_format == 'sparr':
        raise NotImplementedError(
            "output_format='sparr' is the legacy pandas-SparseArray format that the "
            "reference itself no longer supports on pandas 2 (SURVEY App. B.8); use 'lsdf'")
    return df_alleles, df_genes


# ---------------------------------------------------------------------------
# H6: non-coding feature extraction (reference :1187-1243)
# ---------------------------------------------------------------------------
def extract_noncoding(genome_gff, genome_fna, noncoding_out, flanking=(0, 0),
                      allowed_features=['transcript', 'tRNA', 'rRNA', 'misc_binding']):
    """Write the nucleotide sequence of every allowed GFF feature (PATRIC
    flavour: contig column is 'accn|<contig>', 5 characters trimmed, :1221)."""
    contigs = load_sequences_from_fasta(genome_fna, header_fxn=lambda x: x.split()[0])
    with open(noncoding_out, 'w+') as f_out, open(genome_gff, 'r') as f_gff:
        for line in f_gff:
            if line[0] == '#' or len(line.strip()) == 0:
                continue
            contig, _src, ftype, start, stop, _score, strand, _phase, meta = line.split('\t')
            contig = contig[5:]
            start, stop = int(start), int(stop)
            if ftype not in allowed_features or contig not in contigs:
                continue
            lo = max(0, start - 1 - flanking[0])
            seq = contigs[contig][lo:stop + flanking[1]]
            if strand == '-':
                seq = reverse_complement(seq)
            fields = [kv.split('=') for kv in meta.split(';')]
            feature_id = {kv[0]: kv[1] for kv in fields}['ID']
            wrapped = '\n'.join(seq[i:i + 70] for i in range(0, len(seq), 70))
            f_out.write('>' + feature_id + '\n' + wrapped + '\n')


# ---------------------------------------------------------------------------
# the same pipeline on libpgx's host side: consolidate -> cluster -> name -> tables
# ---------------------------------------------------------------------------
def _lex_key(values, shorter_first):
    """Sort key under which non-negative integers order like their decimal strings do inside an
    allele name: digit by digit, and where one string ends the other continues with a digit, the
    shorter one sorts first (`shorter_first`: the name ends there) or last (the cluster number is
    followed by the variant letter 'A', which sorts after every digit: C100 < C10 < C1, reference
    :615)."""
    v = np.asarray(values, dtype=np.int64)
    pow10 = 10 ** np.arange(1, 19, dtype=np.int64)
    nd = np.searchsorted(pow10, v, side='right') + 1             # number of decimal digits
    width = int(nd.max()) if nd.size else 1
    # digits left-aligned to the longest number, padded with zeros where the name ends after the number (a shorter
    # string sorts first: 1 < 10 < 100) and with nines where the letter follows (it sorts after every digit:
    # 19A < 1A, and among equals the longer first: 100A < 10A < 1A); the digit count breaks the ties that
    # padding creates (all lengths are at most 18: 5 bits)
    scale = np.concatenate(([1], pow10))[width - nd]
    if shorter_first:
        return v * scale * 32 + nd
    return ((v + 1) * scale - 1) * 32 + (31 - nd)


class _Beside(object):
    """A step of the pipeline that runs beside the caller's next steps on a thread of its own (the library's file
    work releases the GIL). wait() returns when it is done and raises what it raised."""

    def __init__(self, fn):
        import threading
        self._exc = None

        def run():
            try:
                fn()
            except BaseException as exc:          # handed to the thread that waits
                self._exc = exc
        self._thread = threading.Thread(target=run)
        self._thread.start()

    def wait(self):
        self._thread.join()
        exc, self._exc = self._exc, None
        if exc is not None:
            raise exc


def _native_pipeline(genome_paths, nr_fasta, shared, missing, names_tsv, name, cluster_type, cdhit_args,
                     fastasort_path, cluster_fn=None, after_tables=None):
    """consolidate_seqs -> cluster_with_cdhit -> rename_genes_and_alleles -> build_genetic_feature_tables
    with the file work in libpgx's multi-threaded host code (csrc/ingest.cpp) and the tables from
    arrays instead of per-record dictionaries: the same files, byte for byte, and the same LSDFs as the
    step-by-step functions above (tests/test_host_golden.py pins both against the reference's output).
    Returns None when the fast path does not apply -- inputs the reference's line-by-line semantics
    treat specially (see pgx.h), duplicate genome names, an external fastasort, a multi-process group:
    the caller then runs the step-by-step functions. `cluster_fn(residues, offsets, params)` replaces the
    GPU clustering call in tests (the CPU oracle, or a reader of a given .clstr). `after_tables(tables)` is called once
    the tables exist, while the text outputs may still be being written (the caller's .npz files go there)."""
    import sys
    import time
    from . import _native, cluster
    genomes = [__get_genome_from_filename__(p) for p in genome_paths]
    if fastasort_path or cluster._group is not None or len(set(genomes)) != len(genomes):
        return None
    t_mark = [time.perf_counter()]

    def lap(what):   # PGX_TRACE: wall time of the pipeline's stages
        if os.environ.get('PGX_TRACE'):
            now = time.perf_counter()
            print('[pgx] pipeline: %-28s %8.1f ms' % (what, (now - t_mark[0]) * 1e3), file=sys.stderr)
            t_mark[0] = now
    try:
        fs = _native.FastaSet(genome_paths)
    except _native.PgxError as exc:
        if getattr(exc, 'status', 0) != _native.ERR_NOMEM:
            raise
        print('Note: taking the step-by-step path (%s)' % exc)   # the native ingest holds 2-3x the input in memory
        return None
    lap('ingest (parse, sha256, dedupe)')
    beside = []           # file work in flight: it reads the set's memory, so it is waited for before the set is closed
    try:
        if not fs.simple:
            print('Note: taking the step-by-step path (%s)' % fs.why)
            return None
        # H1 (:336-405); the nr FASTA itself is written once, below, with the allele names (:524-544 rewrites it)
        # (the header files do not depend on the clustering and are written beside it)
        headers_written = _Beside(lambda: fs.write_consolidated(None, shared, missing))
        beside.append(headers_written)
        print('Headers without sequences:', fs.n_missing)
        nucleotide = nr_fasta[-4:].lower() == '.fna'                           # K1/K2 (:425-450)
        params = cluster.params_from_cdhit_args(cdhit_args, 'nt' if nucleotide else 'aa')
        print('Running: libpgx greedy clustering (%s rules) -i %s -o %s -c %g -n %d' % (
            'cd-hit-est' if nucleotide else 'cd-hit', nr_fasta, nr_fasta + '.cdhit', params.identity, params.word_len))
        if cluster_fn is None:      # (nobody reads the work counters here: the library leaves out what only they need)
            cl, mem, iden, strand, n_clusters = cluster.cluster_sequences(fs.residues, fs.offsets, params, want_stats=False)[:5]
        else:
            cl, mem, iden, strand, n_clusters = cluster_fn(fs.residues, fs.offsets, params)[:5]
        print('%9d  finished  %9d  clusters' % (int((cl >= 0).sum()), n_clusters))
        lap('clustering (H2D included)')
        headers_written.wait()
        lap('redundant / missing headers (the rest)')
        prefix = name + '_' + CLUSTER_TYPES[cluster_type]                      # H2 (:453-560)

        def write_outputs():
            fs.write_clustered(cl, mem, iden, strand, nucleotide, prefix, VARIANT_TYPES['allele'],
                               clstr_path=nr_fasta + '.cdhit.clstr', names_path=names_tsv, nr_out_path=nr_fasta + '.tmp')
            os.replace(nr_fasta + '.tmp', nr_fasta)
        unclustered = np.flatnonzero(cl < 0)
        if unclustered.size:
            for h in fs.headers(fs.rep_of_group[unclustered]):
                print('MISSING:', h)

        print('Loadings header-allele mappings...')                            # H4 (:563-680)
        genome_order = sorted(genomes)
        print('Sorting alleles...')
        # rows of the allele table = the clustered sequences in the order of their names, genes = runs of one cluster;
        # records in sorted(path) order, file order inside (:635); a record counts if it has a sequence (:643); a pair
        # (row, genome) is kept where it is inserted first (:649-650) -- one pass over the parsed files in the library
        genome_of_file = np.array([genome_order.index(g) for g in genomes], dtype=np.int64)
        file_order = np.argsort(np.array(genome_paths, dtype=object), kind='stable')
        t = fs.feature_coo(cl, mem, file_order, genome_of_file)
        allele_groups = t['allele_groups']
        lap('tables: coordinates')
        # (the three text files and the rest of the tables need nothing of each other: the files are written meanwhile;
        # started behind the coordinates, which use all cores themselves)
        outputs_written = _Beside(write_outputs)
        beside.append(outputs_written)
        print('Sorting clusters...')
        c_sorted = cl[allele_groups]
        new_gene = np.ones(c_sorted.size, dtype=bool)
        new_gene[1:] = c_sorted[1:] != c_sorted[:-1]
        allele_order = _native.format_labels(prefix, c_sorted, mem[allele_groups], VARIANT_TYPES['allele'])
        gene_order = _native.format_labels(prefix, c_sorted[new_gene])
        lap('tables: names')
        print('Genomes:', len(genome_order))
        print('Clusters:', len(gene_order))
        print('Alleles:', len(allele_order))
        if t['lost_records'].size:
            for h in fs.headers(t['lost_records']):
                print('MISSING:', h)
        print('Building binary matrix...')

        def ones_coo(row, col, shape):
            return scipy.sparse.coo_matrix((np.ones(row.size, dtype=np.int64), (row, col)), shape=shape)
        sp_alleles = ones_coo(t['a_row'], t['a_col'], (len(allele_order), len(genome_order)))
        sp_genes = ones_coo(t['g_row'], t['g_col'], (len(gene_order), len(genome_order)))
        out = (sparse_utils.LightSparseDataFrame(allele_order, genome_order, sp_alleles),
               sparse_utils.LightSparseDataFrame(gene_order, genome_order, sp_genes))
        lap('tables: matrices')
        if cluster_fn is None:
            # Device-resident hand-off: the gene x genome bitmap is built on the GPU straight from the clustering
            # result (rows = cluster numbers; the curves do not depend on the row order) and stays in the context;
            # estimate_pan_core_size(df_genes) on the returned table uses it instead of uploading the table's
            # coordinates, as long as the table is the object returned here and the bitmap is still resident.
            try:
                ctx = _native.default_context()
                token = ctx.bitmap_from_clusters(cl, fs.group_of_record, fs.file_of_record, genome_of_file,
                                                 len(gene_order), len(genome_order))
                # row_cluster: the bitmap row (cluster number) of each table row -- the names sort as strings
                out[1]._pgx_resident = {'ctx': ctx, 'token': token, 'shape': out[1].shape, 'data': out[1].data,
                                        'nnz': int(out[1].data.nnz), 'row_cluster': c_sorted[new_gene].astype(np.int32)}
            except _native.PgxError as exc:       # (the tables are complete without it)
                print('Note: no device-resident bitmap (%s)' % exc)
            lap('device-resident bitmap')
        if after_tables is not None:
            after_tables(out)
        outputs_written.wait()
        lap('.clstr, names, nr FASTA (the rest)')
        return out
    finally:
        for b in beside:
            try:
                b.wait()
            except BaseException:     # (reported by the wait() above unless something else failed first)
                pass
        # (giving back the set's memory, a GB for the benchmark's input, takes 50 ms: nobody waits for it)
        import threading
        threading.Thread(target=fs.close).start()


# ---------------------------------------------------------------------------
# entry points (reference :44-156, :159-316)
# ---------------------------------------------------------------------------
def _save_both(df_alleles, allele_npz, df_genes, gene_npz):
    """The two tables of a pangenome, written side by side (the deflate of the .npz members releases the GIL);
    the messages come in the reference's order."""
    import sys
    import threading
    import time
    t0 = time.perf_counter()
    print('Saving', allele_npz, '...')
    errors = []

    def save_genes():
        try:
            df_genes.to_npz(gene_npz)
        except BaseException as exc:      # re-raised by the caller's thread
            errors.append(exc)
    t = threading.Thread(target=save_genes)
    t.start()
    try:
        df_alleles.to_npz(allele_npz)
    finally:
        print('Saving', gene_npz, '...')
        t.join()
    if errors:
        raise errors[0]
    if os.environ.get('PGX_TRACE'):
        print('[pgx] pipeline: %-28s %8.1f ms' % ('.npz + labels', (time.perf_counter() - t0) * 1e3), file=sys.stderr)


def _check_format(output_format):
    if output_format not in {'lsdf', 'sparr'}:
        print('Unrecognized output format, switching to lsdf')
        return 'lsdf'
    return output_format


def _p(output_dir, name, suffix):
    return (output_dir + '/' + name + suffix).replace('//', '/')


def build_cds_pangenome(genome_faa_paths, output_dir, name='Test',
                        cdhit_args={'-n': 5, '-c': 0.8}, fastasort_path=None,
                        output_format='lsdf'):
    """Protein pan-genome: dedupe -> cluster (HIP) -> name -> tables -> npz.
    Output files and return value as the reference (:44-156)."""
    output_format = _check_format(output_format)
    print('Identifying non-redundant CDS sequences...')
    nr_faa = _p(output_dir, name, '_nr.faa')
    shared = _p(output_dir, name, '_redundant_headers.tsv')
    missing = _p(output_dir, name, '_missing_headers.txt')
    allele_npz = _p(output_dir, name, '_strain_by_allele') + '.npz'
    gene_npz = _p(output_dir, name, '_strain_by_gene') + '.npz'
    fast = _native_pipeline(genome_faa_paths, nr_faa, shared, missing, _p(output_dir, name, '_allele_names.tsv'),
                            name, 'cds', cdhit_args, fastasort_path,
                            after_tables=lambda t: _save_both(t[0], allele_npz, t[1], gene_npz)) \
        if output_format == 'lsdf' else None
    if fast is not None:
        return fast                 # (the tables were saved beside the last of the text outputs)
    else:
        consolidate_seqs(genome_faa_paths, nr_faa, shared, missing)

        cluster_with_cdhit(nr_faa, nr_faa + '.cdhit', cdhit_args)
        os.remove(nr_faa + '.cdhit')
        clstr = nr_faa + '.cdhit.clstr'

        header_to_allele = rename_genes_and_alleles(
            clstr, nr_faa, nr_faa, _p(output_dir, name, '_allele_names.tsv'), name=name,
            cluster_type='cds', shared_headers_file=shared, fastasort_path=fastasort_path)
        df_alleles, df_genes = build_genetic_feature_tables(
            clstr, genome_faa_paths, name, cluster_type='cds',
            output_format=output_format, header_to_allele=header_to_allele)

    allele_npz = _p(output_dir, name, '_strain_by_allele') + '.npz'
    gene_npz = _p(output_dir, name, '_strain_by_gene') + '.npz'
    _save_both(df_alleles, allele_npz, df_genes, gene_npz)
    return df_alleles, df_genes


def build_noncoding_pangenome(genome_data, output_dir, name='Test', flanking=(0, 0),
                              allowed_features=['transcript', 'tRNA', 'rRNA', 'misc_binding'],
                              cdhit_args={'-n': 5, '-c': 0.8}, fastasort_path=None,
                              output_format='lsdf', fna_output_footer='', overwrite_extract=False):
    """Non-coding pan-genome from (gff, fna) pairs; nucleotide clustering
    (cd-hit-est rules) because the merged file ends in .fna (reference :159-316)."""
    output_format = _check_format(output_format)
    print('Extracting non-coding sequences...')
    nc_paths = []
    for i, (gff, fna) in enumerate(genome_data):
        genome = __get_genome_from_filename__(gff)
        gdir = '/'.join(gff.split('/')[:-1]) + '/' if '/' in gff else ''
        nc_dir = gdir + 'derived/'
        if not os.path.exists(nc_dir):
            os.mkdir(nc_dir)
        nc = nc_dir + genome + '_noncoding' + fna_output_footer + '.fna'
        nc_paths.append(nc)
        if os.path.exists(nc) and not overwrite_extract:
            print(i + 1, 'Using pre-existing noncoding sequences for', genome)
        else:
            print(i + 1, 'Extracting noncoding regions for', genome)
            extract_noncoding(gff, fna, nc, flanking=flanking, allowed_features=allowed_features)

    print('Identifying non-redundant non-coding sequences...')
    nr_fna = _p(output_dir, name, '_noncoding_nr.fna')
    shared = _p(output_dir, name, '_noncoding_redundant_headers.tsv')
    missing = _p(output_dir, name, '_noncoding_missing_headers.txt')
    fast = _native_pipeline(nc_paths, nr_fna, shared, missing, _p(output_dir, name, '_noncoding_allele_names.tsv'),
                            name, 'noncoding', cdhit_args, fastasort_path) if output_format == 'lsdf' else None
    if fast is not None:
        df_alleles, df_genes = fast
    else:
        consolidate_seqs(nc_paths, nr_fna, shared, missing)

        cluster_with_cdhit(nr_fna, nr_fna + '.cdhit', cdhit_args)
        os.remove(nr_fna + '.cdhit')
        clstr = nr_fna + '.cdhit.clstr'

        header_to_allele = rename_genes_and_alleles(
            clstr, nr_fna, nr_fna, _p(output_dir, name, '_noncoding_allele_names.tsv'), name=name,
            cluster_type='noncoding', shared_headers_file=shared, fastasort_path=fastasort_path)
        df_alleles, df_genes = build_genetic_feature_tables(
            clstr, nc_paths, name, cluster_type='noncoding',
            output_format=output_format, header_to_allele=header_to_allele)
    # plain lists on purpose; the maps are not refreshed (reference :292-293, App. B.5)
    strip = '_noncoding' + fna_output_footer
    df_alleles.columns = [x.replace(strip, '') for x in df_alleles.columns]
    df_genes.columns = [x.replace(strip, '') for x in df_genes.columns]

    allele_npz = _p(output_dir, name, '_strain_by_noncoding_allele') + '.npz'
    gene_npz = _p(output_dir, name, '_strain_by_noncoding_gene') + '.npz'
    _save_both(df_alleles, allele_npz, df_genes, gene_npz)
    return df_alleles, df_genes

# ---------------------------------------------------------------------------
# proximal (5'/3' UTR) pangenomes (reference :743-1184, :2027-2038)
# ---------------------------------------------------------------------------
# Host-only rows: exact-match grouping per gene instead of clustering, the same table machinery. Mirrored
# statement by statement where Python's own semantics decide the outcome (negative slice starts at contig
# ends, dictionary insertion order, the unconditional last record); tests/golden/proximal holds what the
# reference produced.
def __load_feature_to_allele__(allele_names):
    """{'fig|<genome>.peg.#': allele} from <name>_allele_names.tsv: every synonym of a line, cut to its
    first two '|' fields (reference :2027-2038)."""
    feat_to_allele = {}
    with open(allele_names, 'r') as f:
        for line in f:
            data = line.strip().split('\t')
            for synonym in data[1:]:
                feat_to_allele['|'.join(synonym.split('|')[:2])] = data[0]
    return feat_to_allele


def extract_proximal_sequences(genome_gff, genome_fna, proximal_out, limits, max_overlap, side,
                               feature_to_allele=None, allele_names=None, include_fragments=False, ctx=None):
    """Nucleotides upstream / downstream of every mapped GFF feature (PATRIC flavour: contig column
    'accn|<contig>', ID attribute) written as '<ID>_<side>(<limits>[,<max_overlap>])' records
    (reference :1038-1184). limits = (-X, Y): upstream X bases before the start codon + the first Y coding
    bases; downstream the last X coding bases + Y bases after the stop. max_overlap >= 0 truncates a region
    that runs into the neighbouring CDS on the same strand (GFF order). Regions cut off by a contig end are
    dropped unless include_fragments. ctx (a _native.Context): the windows are cut on the device (csrc/prox.hip,
    DESIGN.md 6k), the file is the same bytes; a genome that is not regular goes through the code below."""
    if ctx is not None:
        _extract_proximal_with_ctx(ctx, genome_gff, genome_fna, proximal_out, limits, max_overlap, side,
                                   feature_to_allele, allele_names, include_fragments)
        return
    neighbours = {}      # contig -> strand -> (start, stop) -> (end of the CDS before, start of the CDS after)
    if max_overlap >= 0:
        placed = {}
        with open(genome_gff, 'r') as f_gff:
            for line in f_gff:
                line = line.strip()
                if len(line) > 0 and line[0] != '#':
                    contig, _src, ftype, start, stop, _score, strand, _phase, _attr = line.split('\t')
                    if ftype == 'CDS':
                        contig = contig.split('|')[-1]
                        placed.setdefault(contig, {'+': [], '-': []})[strand].append((int(start) - 1, int(stop)))
        for contig, by_strand in placed.items():
            neighbours[contig] = {'+': {}, '-': {}}
            for strand, feats in by_strand.items():
                for i, feat in enumerate(feats):
                    left = -np.inf if i == 0 else feats[i - 1][1]
                    right = np.inf if i == len(feats) - 1 else feats[i + 1][0]
                    neighbours[contig][strand][feat] = (left, right)

    contigs = load_sequences_from_fasta(genome_fna, header_fxn=lambda x: x.split()[0])
    if feature_to_allele:
        feat_to_allele = feature_to_allele
    elif allele_names:
        feat_to_allele = __load_feature_to_allele__(allele_names)
    else:
        feat_to_allele = None

    params = (limits[0], limits[1], max_overlap) if max_overlap >= 0 else limits
    footer = '_' + side + str(params).replace(' ', '')
    coding_length = limits[1] if side == 'upstream' else -limits[0]
    count = 0
    with open(proximal_out, 'w+') as f_prox, open(genome_gff, 'r') as f_gff:
        for line in f_gff:
            line = line.strip()
            if len(line) == 0 or line[0] == '#':
                continue
            contig, _src, _ftype, start, stop, _score, strand, _phase, attr_raw = line.split('\t')
            contig = contig.split('|')[-1]
            start, stop = int(start) - 1, int(stop)
            attrs = {}
            for entry in attr_raw.split(';'):
                k, v = entry.split('=')
                attrs[k] = v
            gffid = attrs['ID']
            if contig not in contigs:
                continue
            # (evaluated in the reference's order: without a mapping the membership test itself fails, :1166)
            if not (gffid in feat_to_allele or feat_to_allele is None):
                continue
            seq = contigs[contig]
            anchor = start if (side, strand) in (('upstream', '+'), ('downstream', '-')) else stop
            lo, hi = limits if strand == '+' else (-limits[1], -limits[0])
            utr_start, utr_stop = anchor + lo, anchor + hi
            if max_overlap >= 0:
                left, right = neighbours[contig][strand][(start, stop)]
                if utr_start < left - max_overlap:
                    utr_start = left - max_overlap
                if utr_stop > right + max_overlap:
                    utr_stop = right + max_overlap
            proximal = seq[utr_start:utr_stop].strip()      # (a negative start counts from the contig's end, as there)
            if strand == '-':
                proximal = reverse_complement(proximal)
            is_fragment = utr_start < 0 or utr_stop > len(seq)
            if len(proximal) > coding_length and (not is_fragment or include_fragments):
                f_prox.write('>' + gffid + footer + '\n' + proximal + '\n')
                count += 1
    print('Loaded', side, 'sequences:', count)


def extract_upstream_sequences(genome_gff, genome_fna, upstream_out, limits=(-50, 3), max_overlap=-1,
                               feature_to_allele=None, allele_names=None, include_fragments=False, ctx=None):
    """Reference :1021-1029."""
    extract_proximal_sequences(genome_gff, genome_fna, proximal_out=upstream_out, limits=limits, max_overlap=max_overlap,
                               side='upstream', feature_to_allele=feature_to_allele, allele_names=allele_names,
                               include_fragments=include_fragments, ctx=ctx)


def extract_downstream_sequences(genome_gff, genome_fna, downstream_out, limits=(-3, 50), max_overlap=-1,
                                 feature_to_allele=None, allele_names=None, include_fragments=False, ctx=None):
    """Reference :1032-1040."""
    extract_proximal_sequences(genome_gff, genome_fna, proximal_out=downstream_out, limits=limits, max_overlap=max_overlap,
                               side='downstream', feature_to_allele=feature_to_allele, allele_names=allele_names,
                               include_fragments=include_fragments, ctx=ctx)


def consolidate_proximal(genome_proximals, nr_proximal_out, feature_to_allele, side, output_format='lsdf', ctx=None):
    """Non-redundant proximal sequences PER GENE (<name>_C#U# upstream, <name>_C#D# downstream; the number
    is the order of first appearance within the gene) and the proximal x genome table (reference :900-1018).
    Files are taken in sorted order; the genome is the file name up to '_<side>'. ctx (a _native.Context): the records
    are grouped and numbered on the device (csrc/prox.hip), files and table are the same; a call that is
    not regular goes through the code below."""
    if ctx is not None:
        return _consolidate_proximal_with_ctx(ctx, genome_proximals, nr_proximal_out, feature_to_allele, side, output_format, {})
    letter = VARIANT_TYPES[side]
    variants = {}        # gene -> {sequence: number}
    per_genome = {}      # genome -> {proximal id: 1}, insertion order = first appearance
    genome_order = []
    ids = set()
    with open(nr_proximal_out, 'w+') as f_nr:
        def record(header, seq, genome):
            feature = header.split('_' + side + '(')[0]
            gene = __get_gene_from_allele__(feature_to_allele[feature])
            known = variants.setdefault(gene, {})
            is_new = seq not in known
            if is_new:
                known[seq] = len(known)
            prox_id = gene + letter + str(known[seq])
            ids.add(prox_id)
            per_genome[genome][prox_id] = 1
            if is_new:
                f_nr.write('>' + prox_id + '\n' + seq + '\n')
        for path in sorted(genome_proximals):
            genome = path.split('/')[-1].split('_' + side)[0]
            per_genome[genome] = {}
            genome_order.append(genome)
            header, seq = '', ''
            with open(path, 'r') as f:
                for line in f.readlines():
                    if line[0] == '>':
                        if len(seq) > 0:
                            record(header, seq, genome)
                        header, seq = line[1:].strip(), ''
                    else:
                        seq += line.strip()
            record(header, seq, genome)          # the last record, unconditionally (:975-990)
    print('Sparsifying', side, 'table...')
    prox_order = sorted(ids)
    index_of = {p: i for i, p in enumerate(prox_order)}
    rows, cols = [], []
    for genome_i, genome in enumerate(genome_order):
        for prox_id in per_genome[genome]:
            rows.append(index_of[prox_id])
            cols.append(genome_i)
    print('Building binary matrix...')
    data = _first_occurrence_coo(rows, cols, len(prox_order), len(genome_order))
    if output_format == 'sparr':
        raise NotImplementedError("output_format='sparr' is not supported (SURVEY App. B.8); use 'lsdf'")
    return sparse_utils.LightSparseDataFrame(prox_order, genome_order, data)


def build_proximal_pangenome(genome_data, allele_names, output_dir, limits, side, name='Test',
                             include_fragments=False, max_overlap=-1, fastasort_path=None,
                             output_format='lsdf', fna_output_footer='', overwrite_extract=False, ctx=None):
    """Proximal-region pangenome relative to the gene clusters of build_cds_pangenome(): per genome
    `<gffdir>/derived/<genome>_<side><footer>.fna`, then `<name>_nr_<side>.fna` and
    `<name>_strain_by_<side>.npz` (reference :777-897). ctx (a _native.Context): windows are cut and records grouped
    on the device, and the records of a genome just extracted there are grouped from memory."""
    output_format = _check_format(output_format)
    print('Loading header-allele mapping...')
    feature_to_allele = __load_feature_to_allele__(allele_names)
    print('Extracting', side, 'sequences...')
    genome_proximals = []
    extracted = {}       # ctx: extract path -> the records of a genome just extracted on the device
    for i, (gff, fna) in enumerate(genome_data):
        genome = __get_genome_from_filename__(gff)
        gdir = '/'.join(gff.split('/')[:-1]) + '/' if '/' in gff else ''
        prox_dir = gdir + 'derived/'
        if not os.path.exists(prox_dir):
            os.mkdir(prox_dir)
        prox = prox_dir + genome + '_' + side + fna_output_footer + '.fna'
        genome_proximals.append(prox)
        if os.path.exists(prox) and not overwrite_extract:
            print(i + 1, 'Using pre-existing', side, 'regions for', genome)
        else:
            print(i + 1, 'Extracting', side, 'regions for', genome)
            if ctx is not None:
                extracted.pop(prox, None)
                records = _extract_proximal_with_ctx(ctx, gff, fna, prox, limits, max_overlap, side, feature_to_allele, None,
                                                     include_fragments)
                if records is not None:
                    extracted[prox] = records
                continue
            extract_proximal_sequences(gff, fna, prox, limits=limits, side=side, feature_to_allele=feature_to_allele,
                                       include_fragments=include_fragments, max_overlap=max_overlap)
    print('Identifying non-redundant', side, 'sequences per gene...')
    nr_out = _p(output_dir, name, '_nr_' + side + '.fna')
    if ctx is not None:
        df_proximal = _consolidate_proximal_with_ctx(ctx, genome_proximals, nr_out, feature_to_allele, side, output_format,
                                                     extracted)
    else:
        df_proximal = consolidate_proximal(genome_proximals, nr_out, feature_to_allele, side, output_format=output_format)
    if fastasort_path:
        print('Sorting sequences by header...')
        with open(nr_out + '.tmp', 'w+') as f_sort:
            sp.call(['./' + fastasort_path, nr_out], stdout=f_sort)
        os.rename(nr_out + '.tmp', nr_out)
    npz = _p(output_dir, name, '_strain_by_' + side) + '.npz'
    print('Saving', npz, '...')
    df_proximal.to_npz(npz)
    return df_proximal


def build_upstream_pangenome(genome_data, allele_names, output_dir, limits=(-50, 3), name='Test',
                             include_fragments=False, max_overlap=-1, fastasort_path=None, output_format='lsdf',
                             fna_output_footer='', overwrite_extract=False, ctx=None):
    """5'UTR pangenome (reference :743-757)."""
    return build_proximal_pangenome(genome_data, allele_names, output_dir, limits, side='upstream', name=name,
                                    include_fragments=include_fragments, max_overlap=max_overlap,
                                    fastasort_path=fastasort_path, output_format=output_format,
                                    fna_output_footer=fna_output_footer, overwrite_extract=overwrite_extract, ctx=ctx)


def build_downstream_pangenome(genome_data, allele_names, output_dir, limits=(-3, 50), name='Test',
                               include_fragments=False, max_overlap=-1, fastasort_path=None, output_format='lsdf',
                               fna_output_footer='', overwrite_extract=False, ctx=None):
    """3'UTR pangenome (reference :761-775)."""
    return build_proximal_pangenome(genome_data, allele_names, output_dir, limits, side='downstream', name=name,
                                    include_fragments=include_fragments, max_overlap=max_overlap,
                                    fastasort_path=fastasort_path, output_format=output_format,
                                    fna_output_footer=fna_output_footer, overwrite_extract=overwrite_extract, ctx=ctx)


# ---------------------------------------------------------------------------
# the same builders with ctx=: windows cut and records grouped on the device (csrc/prox.hip). Everything
# here works on whole files as byte arrays -- no statement runs per GFF line, per record or per base (a file's contigs, the
# files and the distinct alleles are looped over). Only REGULAR input is handled: for anything else a function returns None
# before it has written or printed anything, and its caller runs the host function above, called exactly as without ctx,
# so that what an odd input gives -- exceptions and partial files included -- is the host path's by construction.
# ---------------------------------------------------------------------------
PROXIMAL_PATH_COUNTS = collections.Counter()    # extract_device / extract_host per genome, consolidate_device / _host per call
_PROX_MAX_RECORDS, _PROX_MAX_BYTES, _PROX_MAX_GENES = 1 << 24, 1 << 32, 1 << 24     # the limits of pgx_prox_cut / _group
_PROX_SPACE = np.zeros(256, dtype=bool)
_PROX_SPACE[[9, 11, 12, 32]] = True             # what strip() takes off a line of a regular file ('\n' ends it, '\r' is irregular)


def _plain_ascii(data):
    """the rule of _fasta_records, and no NUL (fixed-width numpy strings end at one)"""
    return data.isascii() and data.translate(None, _STR_ONLY_SPACE + b'\x00') == data


def _line_spans(arr):
    """(starts, ends) of the lines of a byte array, the '\n' excluded; a last line without one counts"""
    nl = np.flatnonzero(arr == 10)
    starts = np.concatenate((np.zeros(1, dtype=np.int64), nl + 1))
    ends = np.concatenate((nl, np.array([arr.size], dtype=np.int64)))
    if starts[-1] == arr.size:
        starts, ends = starts[:-1], ends[:-1]
    return starts, ends


def _ragged_index(starts, lens):
    """the indices starts[0] .. starts[0] + lens[0] - 1, starts[1] .., end to end"""
    lens = np.asarray(lens, dtype=np.int64)
    before = np.cumsum(lens) - lens
    return np.repeat(np.asarray(starts, dtype=np.int64) - before, lens) + np.arange(int(lens.sum()), dtype=np.int64)


def _fixed_width(arr, starts, lens):
    """the byte strings arr[starts[i]:starts[i] + lens[i]] as one numpy 'S' array"""
    width = max(int(lens.max()) if lens.size else 0, 1)
    out = np.zeros((lens.size, width), dtype=np.uint8)
    if lens.size:
        rows = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
        out[rows, _ragged_index(np.zeros(lens.size, dtype=np.int64), lens)] = arr[_ragged_index(starts, lens)]
    return out.view('S%d' % width).reshape(-1)


def _decimal_fields(arr, starts, ends):
    """int64 values of fields of plain decimal digits; None if one of them is anything else"""
    lens = ends - starts
    if lens.size == 0:
        return np.zeros(0, dtype=np.int64)
    if int(lens.min()) < 1 or int(lens.max()) > 18:
        return None
    digits = arr[_ragged_index(starts, lens)].astype(np.int64) - 48
    if digits.min() < 0 or digits.max() > 9:
        return None
    place = np.repeat(lens, lens) - 1 - _ragged_index(np.zeros(lens.size, dtype=np.int64), lens)
    return np.add.reduceat(digits * 10 ** place, np.cumsum(lens) - lens)


def _parse_gff_regular(data):
    """The non-comment lines of a GFF file as arrays (one entry per line, file order), or None if the file is not regular:
    arr (the file's bytes), contig (start, end of the name behind the last '|'), is_cds, start0, stop, plus, id (start, end
    of the value of the last ID attribute)."""
    if not _plain_ascii(data):
        return None
    arr = np.frombuffer(data, dtype=np.uint8)
    ls, le = _line_spans(arr)
    full = le > ls
    ls, le = ls[full], le[full]
    if ls.size and (_PROX_SPACE[arr[ls]].any() or _PROX_SPACE[arr[le - 1]].any()):
        return None                                          # (strip() would change the line: leave it to the host)
    keep = arr[ls] != 35 if ls.size else np.zeros(0, dtype=bool)                     # '#'
    ls0, le0 = ls, le
    ls, le = ls[keep], le[keep]
    n = ls.size
    tabs = np.flatnonzero(arr == 9)
    lo = np.searchsorted(tabs, ls)
    if n and (np.searchsorted(tabs, le) - lo != 8).any():
        return None
    t = tabs[lo[:, None] + np.arange(8)[None, :]] if n else np.zeros((0, 8), dtype=np.int64)
    # contig.split('|')[-1]
    pipes = np.flatnonzero(arr == 124)
    c_end = t[:, 0]
    c_start = ls.copy()
    if pipes.size and n:
        j = np.searchsorted(pipes, c_end) - 1
        last = pipes[np.maximum(j, 0)]
        c_start = np.where((j >= 0) & (last >= ls), last + 1, ls)
    ty = t[:, 1] + 1
    at = lambda p: arr[np.minimum(p, arr.size - 1)]                                   # noqa: E731
    is_cds = (t[:, 2] - ty == 3) & (at(ty) == 67) & (at(ty + 1) == 68) & (at(ty + 2) == 83)
    start = _decimal_fields(arr, t[:, 2] + 1, t[:, 3])
    stop = _decimal_fields(arr, t[:, 3] + 1, t[:, 4])
    if start is None or stop is None:
        return None
    strand = at(t[:, 5] + 1)
    if n and ((t[:, 6] - t[:, 5] != 2).any() or ((strand != 43) & (strand != 45)).any()):
        return None
    # the attributes: entries between ';', each with exactly one '=' -- the separators of a line alternate '=', ';', ..., '='
    a_start = t[:, 7] + 1
    seps = np.flatnonzero((arr == 59) | (arr == 61))
    s_lo = np.searchsorted(seps, a_start)
    count = np.searchsorted(seps, le) - s_lo
    if n and (count % 2 != 1).any():
        return None
    sp = seps[_ragged_index(s_lo, count)]
    line = np.repeat(np.arange(n, dtype=np.int64), count)
    k = _ragged_index(np.zeros(n, dtype=np.int64), count)
    if sp.size and (arr[sp] != np.where(k % 2 == 0, 61, 59)).any():
        return None
    is_eq = k % 2 == 0
    before = np.concatenate((np.zeros(1, dtype=np.int64), sp[:-1])) if sp.size else sp
    after = np.concatenate((sp[1:], np.zeros(1, dtype=np.int64))) if sp.size else sp
    entry_start = np.where(k == 0, a_start[line], before + 1)[is_eq]
    value_end = np.where(k == count[line] - 1, le[line], after)[is_eq]
    eq, line = sp[is_eq], line[is_eq]

    def last_value(key):
        """(start, end) of the value of the last entry named `key` of every line, (-1, -1) on a line without one"""
        named = eq - entry_start == len(key)
        for j, ch in enumerate(key):
            named &= at(entry_start + j) == ch
        of_line = line[named]
        final = np.ones(of_line.size, dtype=bool)
        final[:-1] = of_line[1:] != of_line[:-1]             # a later entry replaces an earlier one
        v_start, v_end = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        v_start[of_line[final]], v_end[of_line[final]] = eq[named][final] + 1, value_end[named][final]
        return v_start, v_end
    id_start, id_end = last_value(b'ID')
    if n and int(id_start.min()) < 0:
        return None                                          # a line without ID
    # (a comment line of exactly nine fields is a record for extract_annotations, which does not know comments)
    comments = ~keep
    comment_records = bool(comments.any() and (np.searchsorted(tabs, le0[comments]) - np.searchsorted(tabs, ls0[comments]) == 8).any())
    return dict(arr=arr, n=n, contig=(c_start, c_end), is_cds=is_cds, start0=start - 1, stop=stop, plus=strand == 43,
                id=(id_start, id_end), type=(ty, t[:, 2]), product=last_value(b'product'), locus_tag=last_value(b'locus_tag'),
                comment_records=comment_records)


def _parse_fna_regular(data):
    """(text uint8: the contigs end to end, {name: (offset, length)}) as load_sequences_from_fasta(header_fxn=first token)
    gives them, or None if the file is not regular. The loop is over contigs."""
    if not data.isascii() or (data and data[:1] != b'>'):
        return None
    # one pass over the file: bytes that make it irregular anywhere, and blanks, which may stand in header lines only
    odd = _STR_ONLY_SPACE + b'\x00'
    outside_lines = len(data) - len(data.translate(None, odd + _BYTES_SPACE))
    pieces, where, total = [], {}, 0
    for i, chunk in enumerate(data.split(b'\n>') if data else ()):
        head, _, body = chunk.partition(b'\n')
        if i == 0:
            head = head[1:]                                  # (the file's first '>')
        tokens = head.split()
        if not tokens:
            return None                                      # (no name: IndexError on the host)
        if len(head.translate(None, odd)) != len(head):
            return None
        outside_lines -= len(head) - len(head.translate(None, _BYTES_SPACE))
        seq = body.replace(b'\n', b'')
        if seq:
            where[tokens[0]] = (total, len(seq))             # a later contig of the same name replaces the earlier one
            pieces.append(seq)
            total += len(seq)
    if outside_lines:
        return None                                          # (blanks inside a sequence line: strip() would leave them there)
    return np.frombuffer(b''.join(pieces), dtype=np.uint8), where


def _parse_extract_regular(data, side):
    """The records of a per-genome extract as consolidate_proximal takes them -- (features: list of str, blob uint8: the
    sequences end to end, lengths int64) -- or None if the file is not regular (an empty one is not). A record without a
    sequence is dropped unless it is the file's last; lines before the first header are a record with the feature ''."""
    if not data or not _plain_ascii(data):
        return None
    arr = np.frombuffer(data, dtype=np.uint8)
    ls, le = _line_spans(arr)
    full = le > ls
    first = np.where(full, arr[np.minimum(ls, arr.size - 1)], 10)
    last = np.where(full, arr[np.maximum(le, 1) - 1], 10)
    is_header = first == 62
    if ((_PROX_SPACE[first] | _PROX_SPACE[last]) & ~is_header).any():
        return None                                          # (strip() would change a sequence line: leave it to the host)
    record = np.cumsum(is_header)
    n_records = int(record[-1]) + 1 if record.size else 1
    seq_lines = ~is_header
    lengths = np.bincount(record[seq_lines], weights=(le - ls)[seq_lines], minlength=n_records).astype(np.int64)
    keep = lengths > 0
    keep[-1] = True                                          # the last record, unconditionally
    blob = arr[_ragged_index(ls[seq_lines], (le - ls)[seq_lines])]
    heads = np.char.strip(_fixed_width(arr, ls[is_header] + 1, (le - ls)[is_header] - 1))
    features = np.concatenate((np.array([b''], dtype=heads.dtype), np.char.partition(heads, ('_' + side + '(').encode())[:, 0])) \
        if heads.size else np.array([b''], dtype='S1')
    return list(map(bytes.decode, features[keep].tolist())), blob, lengths[keep]


def _proximal_neighbours(g, contig_names, wanted):
    """For the lines `wanted` (indices) of a parsed GFF: (left, has_left, right, has_right) of the CDS that has the line's
    contig, strand, start and stop -- the end of the CDS before it and the start of the one after it on that contig and
    strand, in file order -- or None where the host's dictionaries would not give that (two CDS with one key, no CDS)."""
    _, contig_id = np.unique(contig_names, return_inverse=True)
    group = contig_id.reshape(-1).astype(np.int64) * 2 + g['plus']
    cds = np.flatnonzero(g['is_cds'])
    keys = np.stack((group, g['start0'], g['stop']), axis=1)
    uniq, inverse = np.unique(keys, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    per_key = np.bincount(inverse[cds], minlength=uniq.shape[0])
    if (per_key > 1).any() or (per_key[inverse[wanted]] == 0).any():
        return None
    order = np.argsort(group[cds], kind='stable')
    grp, start0, stop = group[cds][order], g['start0'][cds][order], g['stop'][cds][order]
    same_as_before = np.zeros(cds.size, dtype=bool)
    same_as_before[1:] = grp[1:] == grp[:-1]
    same_as_next = np.zeros(cds.size, dtype=bool)
    same_as_next[:-1] = same_as_before[1:]
    position = np.empty(cds.size, dtype=np.int64)            # of a CDS (by its place among the CDS lines) in `order`
    position[order] = np.arange(cds.size)
    cds_of_key = np.zeros(uniq.shape[0], dtype=np.int64)
    cds_of_key[inverse[cds]] = np.arange(cds.size)
    at = position[cds_of_key[inverse[wanted]]]
    return (stop[np.maximum(at - 1, 0)], same_as_before[at], start0[np.minimum(at + 1, max(cds.size - 1, 0))], same_as_next[at])


def _extract_proximal_device(ctx, genome_gff, genome_fna, proximal_out, limits, max_overlap, side, feat_to_allele,
                             include_fragments):
    """extract_proximal_sequences for a regular genome: writes the file, prints the count, returns the file's bytes. None
    (nothing written or printed) for a genome that is left to the host."""
    import itertools
    import numbers
    from . import _native
    if feat_to_allele is None or side not in ('upstream', 'downstream') or len(limits) != 2:
        return None
    if not all(isinstance(x, numbers.Integral) and abs(int(x)) < 1 << 40 for x in (limits[0], limits[1], max_overlap)):
        return None
    try:
        with open(genome_gff, 'rb') as f:
            gff_data = f.read()
        with open(genome_fna, 'rb') as f:
            fna_data = f.read()
    except OSError:
        return None
    g = _parse_gff_regular(gff_data)
    contigs = _parse_fna_regular(fna_data) if g is not None else None
    if contigs is None:
        return None
    text, where = contigs
    arr, n = g['arr'], g['n']
    params = (limits[0], limits[1], max_overlap) if max_overlap >= 0 else limits
    footer = '_' + side + str(params).replace(' ', '')
    if not footer.isascii():
        return None
    coding_length = limits[1] if side == 'upstream' else -limits[0]
    contig_names = _fixed_width(arr, g['contig'][0], g['contig'][1] - g['contig'][0])
    id_start, id_len = g['id'][0], g['id'][1] - g['id'][0]
    contig_of = np.fromiter(map({name: i for i, name in enumerate(where)}.get, contig_names.tolist(), itertools.repeat(-1)),
                            dtype=np.int64, count=n)
    ids = list(map(bytes.decode, _fixed_width(arr, id_start, id_len).tolist()))
    mapped = np.fromiter(map(feat_to_allele.__contains__, ids), dtype=bool, count=n)
    wanted = np.flatnonzero((contig_of >= 0) & mapped)
    spans = np.array(list(where.values()), dtype=np.int64).reshape(-1, 2)
    contig_off, contig_len = spans[contig_of[wanted], 0], spans[contig_of[wanted], 1]
    plus, start0, stop = g['plus'][wanted], g['start0'][wanted], g['stop'][wanted]
    anchor = np.where(plus == (side == 'upstream'), start0, stop)
    utr_start = anchor + np.where(plus, limits[0], -limits[1])
    utr_stop = anchor + np.where(plus, limits[1], -limits[0])
    if max_overlap >= 0:
        around = _proximal_neighbours(g, contig_names, wanted)
        if around is None:
            return None
        left, has_left, right, has_right = around
        utr_start = np.where(has_left & (utr_start < left - max_overlap), left - max_overlap, utr_start)
        utr_stop = np.where(has_right & (utr_stop > right + max_overlap), right + max_overlap, utr_stop)
    # seq[utr_start:utr_stop] as Python slices it: a negative index counts from the end, both are clipped into the contig
    lo = np.where(utr_start < 0, np.maximum(utr_start + contig_len, 0), np.minimum(utr_start, contig_len))
    hi = np.where(utr_stop < 0, np.maximum(utr_stop + contig_len, 0), np.minimum(utr_stop, contig_len))
    length = np.maximum(hi - lo, 0)
    is_fragment = (utr_start < 0) | (utr_stop > contig_len)
    written = (length > coding_length) & (~is_fragment | bool(include_fragments))
    cut = written | ~plus                                    # (a minus window that is not written is still checked)
    if int(cut.sum()) >= _PROX_MAX_RECORDS or text.size >= _PROX_MAX_BYTES or int(length[cut].sum()) >= _PROX_MAX_BYTES:
        return None
    try:
        out, out_offsets, bad = ctx.prox_cut(text, (contig_off + lo)[cut], length[cut], ~plus[cut])
    except _native.PgxError as e:
        if getattr(e, 'status', None) != -1:
            raise
        return None                                          # beyond the library's limits
    if bad.any():
        return None                                          # the host raises its KeyError at that record
    keep = written[cut]
    seq_start, seq_len = out_offsets[:-1].astype(np.int64)[keep], length[cut][keep]
    id_start, id_len = id_start[wanted][written], id_len[wanted][written]
    foot = np.frombuffer(footer.encode('ascii'), dtype=np.uint8)
    record_len = 1 + id_len + foot.size + 1 + seq_len + 1
    at = np.cumsum(record_len) - record_len
    image = np.full(int(record_len.sum()), 10, dtype=np.uint8)                       # ('\n' where nothing else goes)
    image[at] = 62
    image[_ragged_index(at + 1, id_len)] = arr[_ragged_index(id_start, id_len)]
    image[(at + 1 + id_len)[:, None] + np.arange(foot.size)[None, :]] = foot[None, :]
    image[_ragged_index(at + 1 + id_len + foot.size + 1, seq_len)] = out[_ragged_index(seq_start, seq_len)]
    image = image.tobytes()
    with open(proximal_out, 'wb') as f:
        f.write(image)
    print('Loaded', side, 'sequences:', int(written.sum()))
    return image


def _extract_proximal_with_ctx(ctx, genome_gff, genome_fna, proximal_out, limits, max_overlap, side, feature_to_allele,
                               allele_names, include_fragments):
    """One genome of extract_proximal_sequences(ctx=...). Returns the records of the file written, as
    _parse_extract_regular gives them, when they came from the device, else None."""
    feat_to_allele = None
    if feature_to_allele:
        feat_to_allele = feature_to_allele
    elif allele_names:
        feat_to_allele = __load_feature_to_allele__(allele_names)
    image = _extract_proximal_device(ctx, genome_gff, genome_fna, proximal_out, limits, max_overlap, side, feat_to_allele,
                                     include_fragments)
    if image is None:
        PROXIMAL_PATH_COUNTS['extract_host'] += 1
        extract_proximal_sequences(genome_gff, genome_fna, proximal_out, limits=limits, max_overlap=max_overlap, side=side,
                                   feature_to_allele=feature_to_allele, allele_names=allele_names,
                                   include_fragments=include_fragments)
        return None
    PROXIMAL_PATH_COUNTS['extract_device'] += 1
    return _parse_extract_regular(image, side)               # (what re-reading the file would give; None: re-read it)


def _proximal_row_order(gene_names, genes, variants, letter):
    """(names, rank): the ids <gene><letter><variant> and the place of each among them sorted as strings"""
    from . import _native
    used = np.unique(genes)
    parts = [gene_names[int(g)].rpartition('C') for g in used]
    prefixes = {p[0] + p[1] for p in parts}
    if len(prefixes) == 1 and all(p[1] and p[2].isascii() and p[2].isdigit() and str(int(p[2])) == p[2] and int(p[2]) < 1 << 31
                                  for p in parts) and next(iter(prefixes)).isascii():
        cluster_of = np.zeros(int(used.max()) + 1 if used.size else 1, dtype=np.int32)
        cluster_of[used] = [int(p[2]) for p in parts]
        names = _native.format_labels(next(iter(prefixes)), cluster_of[genes], variants, letter)
        order = _native.allele_order(cluster_of[genes], variants)
    else:
        names = np.array([gene_names[int(g)] + letter + str(int(v)) for g, v in zip(genes, variants)], dtype=object)
        order = np.array(sorted(range(names.size), key=names.__getitem__), dtype=np.int64)
    rank = np.empty(names.size, dtype=np.int64)
    rank[order] = np.arange(names.size)
    return names, rank


def _consolidate_proximal_device(ctx, genome_proximals, nr_proximal_out, feature_to_allele, side, extracted):
    """consolidate_proximal for a regular call; None (nothing written or printed) for one that is left to the host"""
    import itertools
    from . import _native
    letter = VARIANT_TYPES[side]
    paths = sorted(genome_proximals)
    genome_order = [path.split('/')[-1].split('_' + side)[0] for path in paths]
    if len(set(genome_order)) != len(genome_order):
        return None
    features, blobs, lengths, per_file = [], [], [], []
    for path in paths:
        records = extracted.get(path)
        if records is None:
            try:
                with open(path, 'rb') as f:
                    records = _parse_extract_regular(f.read(), side)
            except OSError:
                return None
            if records is None:
                return None
        features.extend(records[0])
        blobs.append(records[1])
        lengths.append(records[2])
        per_file.append(len(records[0]))
    gene_names, gene_ids, gene_of_allele = [], {}, {}
    for allele in set(feature_to_allele.values()):           # once per distinct allele
        gene = __get_gene_from_allele__(allele)
        if gene not in gene_ids:
            gene_ids[gene] = len(gene_names)
            gene_names.append(gene)
        gene_of_allele[allele] = gene_ids[gene]
    n = len(features)
    genes = np.fromiter(map(gene_of_allele.get, map(feature_to_allele.get, features), itertools.repeat(-1)), dtype=np.int64,
                        count=n)
    if n == 0 or genes.min() < 0:
        return None                                          # a feature without an allele: KeyError on the host
    blob = np.concatenate(blobs)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.concatenate(lengths), out=offsets[1:])
    if n >= _PROX_MAX_RECORDS or blob.size >= _PROX_MAX_BYTES or len(gene_names) >= _PROX_MAX_GENES:
        return None
    if not ''.join(gene_names).isascii():
        return None                                          # (the file is put together as bytes)
    try:
        first, variant, n_distinct = ctx.prox_group(blob, offsets, genes.astype(np.int32))
    except _native.PgxError as e:
        if getattr(e, 'status', None) != -1:
            raise
        return None                                          # beyond the library's limits
    own = first == np.arange(n)
    distinct = np.flatnonzero(own)                           # the records written, in the order they are met
    names, rank = _proximal_row_order(gene_names, genes[distinct], variant[distinct], letter)
    names_s = np.asarray(names).astype('S')
    name_len = np.char.str_len(names_s).astype(np.int64)
    seq_start, seq_len = offsets[:-1].astype(np.int64)[distinct], np.concatenate(lengths)[distinct]
    record_len = 1 + name_len + 1 + seq_len + 1
    at = np.cumsum(record_len) - record_len
    image = np.full(int(record_len.sum()), 10, dtype=np.uint8)
    image[at] = 62
    image[_ragged_index(at + 1, name_len)] = names_s.view(np.uint8)[_ragged_index(
        np.arange(distinct.size, dtype=np.int64) * names_s.dtype.itemsize, name_len)]
    image[_ragged_index(at + 1 + name_len + 1, seq_len)] = blob[_ragged_index(seq_start, seq_len)]
    with open(nr_proximal_out, 'wb') as f:
        f.write(image.tobytes())
    print('Sparsifying', side, 'table...')
    prox_order = np.empty(distinct.size, dtype=object)
    prox_order[rank] = [str(x) for x in np.asarray(names).tolist()]
    rows = rank[(np.cumsum(own) - 1)[first]]
    cols = np.repeat(np.arange(len(paths), dtype=np.int64), per_file)
    print('Building binary matrix...')
    data = _first_occurrence_coo(rows, cols, distinct.size, len(genome_order))
    return sparse_utils.LightSparseDataFrame(prox_order.tolist(), genome_order, data)


def _consolidate_proximal_with_ctx(ctx, genome_proximals, nr_proximal_out, feature_to_allele, side, output_format, extracted):
    df = None
    if output_format != 'sparr':                             # (still NotImplementedError, raised where the host raises it)
        df = _consolidate_proximal_device(ctx, genome_proximals, nr_proximal_out, feature_to_allele, side, extracted)
    if df is None:
        PROXIMAL_PATH_COUNTS['consolidate_host'] += 1
        return consolidate_proximal(genome_proximals, nr_proximal_out, feature_to_allele, side, output_format=output_format)
    PROXIMAL_PATH_COUNTS['consolidate_device'] += 1
    return df


# ---------------------------------------------------------------------------
# gene table against allele table, dominant alleles (reference :1246-1330, :1812-1889, helpers :1919-2001):
# runs of allele rows on the device bitmap (csrc/runs.hip)
# ---------------------------------------------------------------------------
def load_feature_table(feature_table):
    """A path ending in .csv / .csv.gz is read with read_csv(index_col=0), one ending in .pickle / .pickle.gz with
    read_pickle; any other string and anything that is not a string comes back as it is (reference :1919-1935)."""
    if isinstance(feature_table, str):
        import pandas as pd
        lower = feature_table.lower()
        if lower.endswith(('.csv', '.csv.gz')):
            return pd.read_csv(feature_table, index_col=0)
        if lower.endswith(('.pickle', '.pickle.gz')):
            return pd.read_pickle(feature_table)
    return feature_table


def breakdown_feature_name(feature_name):
    """(name, cluster type, cluster number, variant type, variant number) of a feature name; the last two are None for a
    cluster-level name (reference :1972-1989).
    Example 1: EsC_A123U56 -> ('EsC', 'A', 123, 'U', 56)
    Example 2: PsA_T789 -> ('PsA', 'T', 789, None, None)"""
    parts = feature_name.split('_')
    name, footer = '_'.join(parts[:-1]), parts[-1]
    for i in range(1, len(footer)):
        if footer[i] in _VARIANT_LETTERS:
            return name, footer[0], int(footer[1:i]), footer[i], int(footer[i + 1:])
    return name, footer[0], int(footer[1:]), None, None


_VARIANT_LETTERS = frozenset(VARIANT_TYPES.values())


def trim_variant(feature_name):
    """The name up to, not including, its right-most alphabetic character (the first character is never looked at); a name
    without one comes back whole (reference :1992-2001)."""
    for i in range(1, len(feature_name)):
        if feature_name[-i].isalpha():
            return feature_name[:-i]
    return feature_name


def _load_table(table):
    """A table argument of the checks below: an .npz path is an LSDF, other paths go through load_feature_table."""
    if isinstance(table, str) and table.lower().endswith('.npz'):
        return sparse_utils.read_lsdf(table)
    return load_feature_table(table)


def _table_cells(table, who, notna):
    """(rows int32, cols int32, index labels, column labels) of the cells of `table` that count as present.
    LightSparseDataFrame: its stored entries, which must all be 1 (the rule of sparse_utils._screen_table: a stored zero or
    any other value raises ValueError rather than being interpreted). pandas frame: with notna, every cell that is not NaN
    (a 0.0 is present: dropna()); otherwise NaN and 0 are absent, 1 is present and any other value raises ValueError."""
    if isinstance(table, sparse_utils.LightSparseDataFrame):
        rows, cols, _, _ = sparse_utils._screen_table(table, who)
        return rows, cols, np.asarray(table.index), np.asarray(table.columns)
    if not (hasattr(table, 'index') and hasattr(table, 'columns') and hasattr(table, 'values')):
        raise TypeError(who + ' takes a LightSparseDataFrame or a pandas DataFrame')
    try:
        values = np.asarray(table.values, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(who + ' needs a numeric table')
    present = ~np.isnan(values)
    if not notna:
        ones = values == 1
        if not np.all(ones | (values == 0) | ~present):
            raise ValueError(who + ' needs a binary table (NaN or 0 = absent, 1 = present)')
        present = ones
    rows, cols = np.nonzero(present)
    return rows.astype(np.int32), cols.astype(np.int32), np.asarray(table.index), np.asarray(table.columns)


def _genes_of_alleles(allele_labels):
    """__get_gene_from_allele__ of every label, as one array operation."""
    labels = np.asarray(allele_labels, dtype=str)
    if labels.size == 0:
        return labels
    return np.char.rpartition(labels, 'A')[:, 0]


def _runs_by_name(gene_labels, allele_genes):
    """validate_gene_table's grouping, whatever the order of the allele rows: one run per gene row (empty when the gene has
    no allele), then one run without a gene row per gene name that occurs only among the alleles, in order of first
    appearance. Returns (run names, run_start uint32, gene_of_run int32, new_row) where new_row[i] is the row allele i gets
    in the gene-sorted table the device sees (a stable relabelling)."""
    gene_labels = np.asarray(gene_labels, dtype=str)
    n_genes = gene_labels.size
    if np.unique(gene_labels).size != n_genes:
        raise ValueError('validate_gene_table needs a gene table without repeated row labels')
    names, first, inverse = np.unique(allele_genes, return_index=True, return_inverse=True)
    order = np.argsort(gene_labels, kind='stable')
    at = np.searchsorted(gene_labels[order], names)
    known = (at < n_genes) & (gene_labels[order][np.minimum(at, max(n_genes - 1, 0))] == names) if n_genes else \
        np.zeros(names.size, dtype=bool)
    run_of_name = np.empty(names.size, dtype=np.int64)
    run_of_name[known] = order[at[known]]
    extra = np.flatnonzero(~known)
    extra = extra[np.argsort(first[extra], kind='stable')]
    run_of_name[extra] = n_genes + np.arange(extra.size)
    run_of_allele = run_of_name[inverse.ravel()] if names.size else np.zeros(0, dtype=np.int64)
    n_runs = n_genes + extra.size
    run_start = np.zeros(n_runs + 1, dtype=np.int64)
    np.cumsum(np.bincount(run_of_allele, minlength=n_runs), out=run_start[1:])
    new_row = np.empty(run_of_allele.size, dtype=np.int64)
    new_row[np.argsort(run_of_allele, kind='stable')] = np.arange(run_of_allele.size)
    gene_of_run = np.full(n_runs, -1, dtype=np.int32)
    gene_of_run[:n_genes] = np.arange(n_genes)
    return np.concatenate([gene_labels, names[extra]]), run_start.astype(np.uint32), gene_of_run, new_row


def _runs_in_order(names):
    """The table-order grouping: maximal stretches of consecutive rows with the same name, so a name may recur.
    Returns (run names, run_start uint32)."""
    names = np.asarray(names, dtype=str)
    if names.size == 0:
        return names, np.zeros(1, dtype=np.uint32)
    starts = np.concatenate([[0], np.flatnonzero(names[1:] != names[:-1]) + 1])
    return names[starts], np.concatenate([starts, [names.size]]).astype(np.uint32)


def _bitmap_row(bits, r):
    """bool [n_genomes]: row r of a bitmap in the library's layout."""
    return ((bits[:, r >> 6] >> np.uint64(r & 63)) & np.uint64(1)).astype(bool)


def _allele_runs(ctx, who, **kwargs):
    from . import _native
    ctx = ctx or _native.default_context()
    out, dups = ctx.allele_runs(**kwargs)
    if any(dups):
        raise ValueError(who + ' needs tables without duplicate entries')
    return out


def validate_gene_table(df_genes, df_alleles, log_group=1, ctx=None):
    """Is the gene x genome table the OR of the allele x genome table's rows, gene by gene? Prints, per genome, the genes on
    which the two tables disagree and returns their number (the reference, :1246-1277, returns None; its printed lines are
    kept, the order of a set's elements apart). Alleles are grouped by __get_gene_from_allele__, whatever their order.
    Both tables may be LightSparseDataFrames (what build_cds_pangenome returns), pandas frames or paths.
    Presence: in a pandas frame every cell that is not NaN, so an explicit 0.0 is present (the reference's dropna()); in
    an LSDF the stored entries, which must all be 1 -- the rule sparse_utils._screen_table applies: a stored zero or any
    other value raises ValueError. The OR, the comparison and the counts run on the device (csrc/runs.hip); names are looked
    up only for the genomes on which something differs. There is no CPU fallback."""
    who = 'validate_gene_table'
    g_rows, g_cols, gene_labels, genomes = _table_cells(_load_table(df_genes), who, notna=True)
    a_rows, a_cols, allele_labels, allele_genomes = _table_cells(_load_table(df_alleles), who, notna=True)
    if not np.array_equal(genomes, allele_genomes):                       # the reference reads dfa[genome] by label
        column_of = {label: j for j, label in enumerate(allele_genomes.tolist())}
        for genome in genomes.tolist():
            if genome not in column_of:
                raise KeyError(genome)
        new_col = np.full(allele_genomes.size, -1, dtype=np.int64)
        new_col[[column_of[g] for g in genomes.tolist()]] = np.arange(genomes.size)
        keep = new_col[a_cols] >= 0
        a_rows, a_cols = a_rows[keep], new_col[a_cols][keep]
    run_names, run_start, gene_of_run, new_row = _runs_by_name(gene_labels, _genes_of_alleles(allele_labels))
    print('Validating gene clusters...')
    out = None
    if genomes.size and run_names.size:
        out = _allele_runs(ctx, who, allele_rows=new_row[a_rows], allele_genomes=a_cols, n_alleles=allele_labels.size,
                           n_genomes=genomes.size, run_start=run_start, gene_rows=g_rows, gene_genomes=g_cols,
                           n_genes=gene_labels.size, gene_of_run=gene_of_run, want=('diff', 'diff_per_genome'))
    num_inconsistencies = 0
    for g, genome in enumerate(genomes.tolist()):
        if (g + 1) % log_group == 0:
            print(g + 1, 'Testing', genome)
        if out is not None and out['diff_per_genome'][g]:
            word = np.flatnonzero(out['diff'][g])
            runs = [int(w) * 64 + b for w in word for b in range(64) if (int(out['diff'][g, w]) >> b) & 1]
            print('\tInconsistent:', set(run_names[runs].tolist()))
            num_inconsistencies += len(runs)
    print('Gene Table Inconsistencies:', num_inconsistencies)
    return num_inconsistencies


def validate_gene_table_dense(df_genes, df_alleles, ctx=None):
    """The row-by-row form of the same check (reference :1280-1330): a run is a maximal stretch of consecutive allele rows
    with the same gene name IN TABLE ORDER (a gene may recur), and the OR of its rows is compared with that gene's row,
    genome by genome in column order. NaN and 0 are absent, 1 is present, any other value raises ValueError; a run whose
    gene is missing from df_genes raises KeyError, as .loc does. The output is the reference's, its quirk included: after
    `Inconsistent` it prints the name of the NEXT run (of the run itself for the last one), then the derived and the stored
    row. Returns the number of inconsistent runs (the reference returns None). Runs on the device (csrc/runs.hip)."""
    who = 'validate_gene_table_dense'
    dfg = _load_table(df_genes)
    g_rows, g_cols, gene_labels, genomes = _table_cells(dfg, who, notna=False)
    a_rows, a_cols, allele_labels, allele_genomes = _table_cells(_load_table(df_alleles), who, notna=False)
    if genomes.size != allele_genomes.size:
        raise ValueError(who + ' compares the tables column by column: they must have as many')
    run_names, run_start = _runs_in_order(_genes_of_alleles(allele_labels))
    if run_names.size == 0:
        raise KeyError(None)             # (the reference ends in dfg.loc[None] on a table without alleles)
    row_of_gene = {}
    for i, label in enumerate(gene_labels.tolist()):
        row_of_gene.setdefault(label, i)
    gene_of_run = np.empty(run_names.size, dtype=np.int32)
    for r, label in enumerate(run_names.tolist()):
        if label not in row_of_gene:
            raise KeyError(label)
        gene_of_run[r] = row_of_gene[label]
    print('Validating gene clusters...')
    out = _allele_runs(ctx, who, allele_rows=a_rows, allele_genomes=a_cols, n_alleles=allele_labels.size,
                       n_genomes=genomes.size, run_start=run_start, gene_rows=g_rows, gene_genomes=g_cols,
                       n_genes=gene_labels.size, gene_of_run=gene_of_run, want=('derived', 'diff', 'diff_per_run'))
    n_runs = run_names.size
    inconsistencies = 0
    marks = set(np.flatnonzero(out['diff_per_run']).tolist())
    marks.update(range(999, n_runs - 1, 1000))
    for r in sorted(marks):
        if out['diff_per_run'][r]:
            has_gene = _bitmap_row(out['derived'], r)
            print('Inconsistent', run_names[min(r + 1, n_runs - 1)])
            print(has_gene)
            if isinstance(dfg, sparse_utils.LightSparseDataFrame):
                print((has_gene != _bitmap_row(out['diff'], r)).astype(np.float64))
            else:
                print(dfg.iloc[int(gene_of_run[r])].fillna(0).values)
            inconsistencies += 1
        if r < n_runs - 1 and (r + 1) % 1000 == 0:
            print('\tTested', r + 1, 'clusters')
    print('Gene Table Inconsistencies:', inconsistencies)
    return inconsistencies


def _gene_name_of_allele(allele):
    terms = breakdown_feature_name(allele)
    return terms[0] + '_' + terms[1] + str(terms[2])


def extract_dominant_alleles(allele_table, allele_faa_file, dominant_out, ctx=None):
    """The most common allele of every gene of an allele x genome table (reference :1812-1889). Runs are maximal stretches of
    consecutive allele rows of one gene in table order; an allele's count is its row sum (NaN and 0 absent, 1 present, any
    other value raises ValueError; an LSDF by its stored entries, all 1); the first allele with the largest count wins;
    genes whose alleles occur nowhere are dropped. Returns df_dominant (index `gene`; columns dominant_allele, gene_count,
    allele_count, the counts float64 as the reference produces them) and writes the dominant alleles' records of
    allele_faa_file to dominant_out. allele_table may be a path (.npz: an LSDF; else load_feature_table). Sums and maxima
    run on the device (csrc/runs.hip); the gene names are parsed from the labels on the host."""
    import pandas as pd
    who = 'extract_dominant_alleles'
    print('Setting up allele table...')
    a_rows, a_cols, allele_labels, genomes = _table_cells(_load_table(allele_table), who, notna=False)
    print('Identifying dominant alleles...')
    run_names, run_start = _runs_in_order([_gene_name_of_allele(a) for a in allele_labels.tolist()])
    columns = ['gene', 'dominant_allele', 'gene_count', 'allele_count']
    df_dominant = pd.DataFrame([], columns=columns)
    if run_names.size and genomes.size:
        out = _allele_runs(ctx, who, allele_rows=a_rows, allele_genomes=a_cols, n_alleles=allele_labels.size,
                           n_genomes=genomes.size, run_start=run_start, want=('total', 'best_allele', 'best_count'))
        kept = np.flatnonzero(out['total'] > 0)
        if kept.size:
            df_dominant = pd.DataFrame({'gene': run_names[kept].tolist(),
                                        'dominant_allele': allele_labels[out['best_allele'][kept]].tolist(),
                                        'gene_count': out['total'][kept].astype(np.float64),
                                        'allele_count': out['best_count'][kept].astype(np.float64)}, columns=columns)
    df_dominant = df_dominant.set_index('gene')
    dominant_alleles = set(df_dominant.dominant_allele.values)
    print('Found dominant alleles', df_dominant.shape, len(dominant_alleles))
    print('Exporting dominant alleles...', end=' ')
    alleles_written = 0
    write_seq = False
    with open(allele_faa_file, 'r') as f_allele, open(dominant_out, 'w+') as f_dom:
        for line in f_allele:
            if line[0] == '>':
                write_seq = line[1:].strip() in dominant_alleles
                alleles_written += write_seq
            if write_seq:
                f_dom.write(line)
    print(alleles_written)
    return df_dominant


# ---------------------------------------------------------------------------
# UTR tables against the genomes (reference :1549-1647): the table's sequences are searched in every contig and its
# reverse complement -- one window scan per genome on the device (csrc/scan.hip)
# ---------------------------------------------------------------------------
_COMPLEMENT_BYTES = ''.join(sorted(_COMPLEMENT_KEYS)).encode('ascii')
SCAN_MAX_WINDOW = 1024             # csrc/scan.hip


def _check_contig(contig):
    """The contig as bytes; KeyError(first character outside the complement table), which is what the reference's
    reverse_complement(contig) raises (:1621)."""
    try:
        raw = contig.encode('ascii')
    except UnicodeEncodeError:
        raw = None
    if raw is None or raw.translate(None, _COMPLEMENT_BYTES):
        reverse_complement(contig)          # raises KeyError(base)
    return raw


def _scan_keys(sequences, window):
    """The keys of one window scan: (keys uint8 [n_keys, window], forward, reverse) for `sequences`, distinct strings of
    length `window`. forward[i] / reverse[i] are the rows of sequence i and of its reverse complement, -1 for none: a
    sequence that is not ASCII has no forward key (no checked contig holds such a character), one with a character outside
    the complement table no reverse key (it cannot occur in a reverse complement). Equal byte strings share one row
    (palindromes; P == rc(Q)). A key holding the byte 0x00, which joins the contigs, raises ValueError."""
    row_of = {}
    forward = np.full(len(sequences), -1, dtype=np.int64)
    reverse = np.full(len(sequences), -1, dtype=np.int64)
    for i, seq in enumerate(sequences):
        try:
            raw = seq.encode('ascii')
        except UnicodeEncodeError:
            continue
        if b'\x00' in raw:
            raise ValueError('a table sequence holds the byte 0x00')
        forward[i] = row_of.setdefault(raw, len(row_of))
        if not raw.translate(None, _COMPLEMENT_BYTES):
            reverse[i] = row_of.setdefault(seq.translate(_COMPLEMENT)[::-1].encode('ascii'), len(row_of))
    keys = np.frombuffer(b''.join(row_of), dtype=np.uint8).reshape(len(row_of), window)
    return keys, forward, reverse


def _short_sequence_found(seq, contigs):
    """The reference's slices at a contig's end are shorter than the window (contig[i:i+window] near len(contig)), so a
    sequence SHORTER than the window matches iff it is a suffix of a contig or of a contig's reverse complement.
    `contigs` have passed _check_contig."""
    m = len(seq)
    for contig in contigs:
        if len(contig) >= m and (contig.endswith(seq) or contig[:m].translate(_COMPLEMENT)[::-1] == seq):
            return True
    return False


def _genome_missing(sequences, contigs, window, scan):
    """found (list of bool) for the distinct table sequences of one genome. scan(text, keys) -> found per key."""
    raws = [_check_contig(c) for c in contigs]
    found = [False] * len(sequences)
    full = [i for i, seq in enumerate(sequences) if len(seq) == window]
    for i, seq in enumerate(sequences):
        if len(seq) < window:
            found[i] = _short_sequence_found(seq, contigs)
    if full and raws:
        keys, forward, reverse = _scan_keys([sequences[i] for i in full], window)
        if keys.shape[0]:
            hit = np.concatenate([np.asarray(scan(b'\x00'.join(raws), keys), dtype=bool), [False]])   # (-1: the last one)
            for i, ok in zip(full, (hit[forward] | hit[reverse]).tolist()):
                found[i] = ok
    return found


def validate_proximal_table_direct(df_prox, genome_fna_paths, nr_prox_fna, limits, side, log_group=1, ctx=None):
    """Partial validation of a proximal x genome table (reference :1573-1647): every sequence the table records for a genome
    must occur in one of the genome's contigs or in a contig's reverse complement; then the start (upstream) or stop
    (downstream) codons among the non-redundant sequences are counted. It does not check WHERE a sequence occurs.
    The printed output is the reference's; the return value is the number of `Missing` lines (the reference returns None).

    df_prox: LightSparseDataFrame (what build_upstream_pangenome returns; its stored entries, which must all be 1), pandas
    frame (every cell that is not NaN, :1612) or a path. genome_fna_paths are taken in the given order; a genome that is no
    column raises KeyError(genome), a recorded row that is not in nr_prox_fna KeyError(label), a contig character outside the
    complement table KeyError(character) -- each where the reference raises it, after that genome's `Evaluating` line.
    Rows of a genome that share a sequence are reported once, at the place of the first and under the name of the last.
    The reference compares the slices contig[i:i+window], window = limits[1] - limits[0], which are shorter at a contig's
    end ("does not yet support non-fixed length UTRs"): a sequence of exactly `window` characters matches wherever it
    occurs -- the device's work, one exact multi-pattern scan per genome (csrc/scan.hip) over the contigs joined by a 0x00
    byte, the reverse strand being searched through the reverse complements of the keys; a shorter sequence matches only as
    the suffix of a contig or of its reverse complement; a longer one never. window must be 1..1024 (ValueError). The next
    genome's FNA is parsed on a host thread while the device scans. There is no CPU fallback."""
    import collections
    from concurrent.futures import ThreadPoolExecutor
    who = 'validate_proximal_table_direct'
    rows, cols, labels, columns = _table_cells(_load_table(df_prox), who, notna=True)
    window = limits[1] - limits[0]
    if not 1 <= window <= SCAN_MAX_WINDOW:
        raise ValueError(who + ' needs 1 <= limits[1] - limits[0] <= %d' % SCAN_MAX_WINDOW)
    order = np.lexsort((rows, cols))
    rows, cols = rows[order], cols[order]
    col_start = np.searchsorted(cols, np.arange(columns.size + 1))
    column_of = {}
    for j, label in enumerate(columns.tolist()):
        column_of.setdefault(label, j)
    labels = labels.tolist()

    print('Loading', side, 'sequences...')
    nr_prox = load_sequences_from_fasta(nr_prox_fna)

    def scan(text, keys):
        nonlocal ctx
        if ctx is None:
            from . import _native
            ctx = _native.default_context()
        return ctx.window_scan(text, keys)

    missing = 0
    genome_fna_paths = list(genome_fna_paths)
    with ThreadPoolExecutor(max_workers=1) as pool:
        ahead = pool.submit(load_sequences_from_fasta, genome_fna_paths[0]) if genome_fna_paths else None
        for g, genome_fna in enumerate(genome_fna_paths):
            genome_contigs = ahead.result()
            ahead = pool.submit(load_sequences_from_fasta, genome_fna_paths[g + 1]) if g + 1 < len(genome_fna_paths) else None
            genome = __get_genome_from_filename__(genome_fna)
            if (g + 1) % log_group == 0:
                print(g + 1, 'Evaluating', genome, genome_fna)
            if genome not in column_of:
                raise KeyError(genome)
            j = column_of[genome]
            table_prox_seqs = {}                       # sequence -> name: first row's place, last row's name (:1613)
            for r in rows[col_start[j]:col_start[j + 1]].tolist():
                table_prox_seqs[nr_prox[labels[r]]] = labels[r]
            sequences = list(table_prox_seqs)
            found = _genome_missing(sequences, list(genome_contigs.values()), window, scan)
            for seq, ok in zip(sequences, found):
                if not ok:
                    print('\tMissing', table_prox_seqs[seq], 'from', genome)
                    missing += 1

    if limits[1] >= 3 and side == 'upstream':
        print('Computing start codon distribution...')
        if limits[1] == 3:
            get_start = lambda x: x[-3:]
        else:
            get_start = lambda x: x[-limits[1]:-limits[1] + 3]
        print(collections.Counter(map(get_start, nr_prox.values())))
    elif limits[0] <= -3 and side == 'downstream':
        print('Computing stop codon distribution...')
        if limits[0] == -3:
            get_stop = lambda x: x[:3]
        else:
            get_stop = lambda x: x[-limits[0] - 3:-limits[0]]
        print(collections.Counter(map(get_stop, nr_prox.values())))
    return missing


def validate_upstream_table_direct(df_upstream, genome_fna_paths, nr_upstream_fna, limits=(-50, 3), log_group=1, ctx=None):
    """validate_proximal_table_direct(..., side='upstream') (reference :1549-1558, which calls the undefined name
    validate_proximal_table and so always raises NameError; here the wrapper calls the function that exists). Returns the
    number of missing sequences."""
    return validate_proximal_table_direct(df_upstream, genome_fna_paths, nr_upstream_fna, limits, 'upstream', log_group, ctx)


def validate_downstream_table_direct(df_downstream, genome_fna_paths, nr_downstream_fna, limits=(-3, 50), log_group=1,
                                     ctx=None):
    """validate_proximal_table_direct(..., side='downstream') (reference :1561-1570, with the same NameError as the upstream
    wrapper; fixed in the same way). Returns the number of missing sequences."""
    return validate_proximal_table_direct(df_downstream, genome_fna_paths, nr_downstream_fna, limits, 'downstream', log_group,
                                          ctx)


# ---------------------------------------------------------------------------
# a table against the FASTA files it was built from (reference :1333-1546): every record of every genome is looked up among
# the non-redundant sequences -- exact look-ups of whole byte strings on the device (csrc/dict.hip) -- and
# the names found are compared with the table's column as two bitmaps
# ---------------------------------------------------------------------------
TABLE_FASTA_BATCH_BYTES = 256 << 20     # key bytes of the genomes whose records share one dict_query call
_TABLE_FASTA_AHEAD = 8                  # genomes parsed ahead of the one being assembled
_STR_ONLY_SPACE = bytes(range(0x1c, 0x20)) + b'\r'   # what str.strip() / universal newlines treat differently from bytes
_BYTES_SPACE = b' \t\x0b\x0c'


def _fasta_records(path):
    """(headers: list of str, sequences: list of bytes) of the records of a FASTA file as validate_table_against_fasta reads
    it (:1480-1489, :1521-1530): text mode, a record starts at a line whose first character is '>', its header is
    line[1:].strip() -- the whole line -- and its sequence the stripped lines joined (as UTF-8 here: the reference hashes
    seq.encode('utf-8')). Lines before the first '>' are a record with the header ''; a record without any line is skipped,
    one whose lines are all blank has the sequence ''. A file of plain ASCII without carriage returns and without the
    separators 0x1c-0x1f, which only str.strip() strips, is cut up as bytes; any other goes through Python's text layer."""
    with open(path, 'rb') as f:
        data = f.read()
    if not data.isascii() or data.translate(None, _STR_ONLY_SPACE) != data:
        return _fasta_records_text(path)
    headers, seqs = [], []
    if not data:
        return headers, seqs
    chunks = data.split(b'\n>')
    if data[:1] == b'>':
        chunks[0] = chunks[0][1:]
    else:
        chunks[0] = b'\n' + chunks[0]                     # an empty header line in front of the leading lines
    if chunks[-1].endswith(b'\n'):
        chunks[-1] = chunks[-1][:-1]                      # the file's last newline ends a line, it does not begin one
    for chunk in chunks:
        nl = chunk.find(b'\n')
        if nl < 0:
            continue                                      # a header and no line
        body = chunk[nl + 1:]
        if body.translate(None, _BYTES_SPACE) == body:
            seqs.append(body.replace(b'\n', b''))
        else:
            seqs.append(b''.join([line.strip() for line in body.split(b'\n')]))
        headers.append(chunk[:nl].strip().decode('ascii'))
    return headers, seqs


def _fasta_records_text(path):
    """_fasta_records through Python's text-mode reading and str.strip(), statement by statement as the reference."""
    headers, seqs = [], []
    with open(path, 'r') as f:
        header, blocks = '', []
        for line in f:
            if line[0] == '>':
                if blocks:
                    headers.append(header)
                    seqs.append(''.join(blocks).encode('utf-8'))
                header, blocks = line[1:].strip(), []
            else:
                blocks.append(line.strip())
        if blocks:
            headers.append(header)
            seqs.append(''.join(blocks).encode('utf-8'))
    return headers, seqs


def _feature_to_allele(allele_names):
    """feature -> allele of an allele names file (:1453-1466): allele TAB feature TAB feature ...; a feature with exactly
    two '|' loses everything from the last one (PATRIC's locus tags); the last line that names a feature wins."""
    out = {}
    with open(allele_names, 'r') as f:
        for line in f:
            data = line.strip().split('\t')
            for feature in data[1:]:
                if feature.count('|') == 2:
                    feature = feature[:feature.rindex('|')]
                out[feature] = data[0]
    return out


def _cells_equal_to_one(table, who):
    """(rows, cols, index labels, column labels) of the cells validate_table_against_fasta counts as present: a
    LightSparseDataFrame by the rule of _table_cells (stored entries, all 1); of a pandas frame the cells that == 1, any
    other value and NaN being absent and nothing raised (the reference's df_ga == 1, :1538)."""
    if isinstance(table, sparse_utils.LightSparseDataFrame):
        return _table_cells(table, who, notna=False)
    if not (hasattr(table, 'index') and hasattr(table, 'columns') and hasattr(table, 'values')):
        raise TypeError(who + ' takes a LightSparseDataFrame or a pandas DataFrame')
    rows, cols = np.nonzero(np.asarray(table.values == 1, dtype=bool).reshape(len(table.index), len(table.columns)))
    return rows.astype(np.int32), cols.astype(np.int32), np.asarray(table.index), np.asarray(table.columns)


def _blob(strings):
    """(blob uint8, offsets uint64 [n + 1]) of a list of bytes objects"""
    offsets = np.zeros(len(strings) + 1, dtype=np.uint64)
    if strings:
        np.cumsum(np.fromiter(map(len, strings), dtype=np.uint64, count=len(strings)), out=offsets[1:])
    return np.frombuffer(b''.join(strings), dtype=np.uint8), offsets


def _genome_keys(path, feature_to_allele, suffix_of):
    """The look-up keys of a genome file's records (:1494-1504): the sequence, and where the record's header -- cut at
    '_upstream(' and then at '_downstream(' -- is a known feature, the sequence + trim_variant(its allele)."""
    headers, seqs = _fasta_records(path)
    if feature_to_allele is not None:
        for i, header in enumerate(headers):
            allele = feature_to_allele.get(header.split('_upstream(')[0].split('_downstream(')[0])
            if allele is not None:
                suffix = suffix_of.get(allele)
                if suffix is None:
                    suffix = suffix_of[allele] = trim_variant(allele).encode('utf-8')
                seqs[i] = seqs[i] + suffix
    return seqs


def validate_table_against_fasta(df_features, genome_fasta_paths, features_fasta, allele_names=None, log_group=1, ctx=None):
    """Verifies that a feature x genome table holds, for every genome, exactly the features whose sequences the genome's
    FASTA file holds (reference :1418-1546): CDS or non-coding allele tables against the FAA / FNA files they were built
    from, and with allele_names (the file build_cds_pangenome writes) upstream / downstream tables against the extracted
    UTR files, where sequence AND gene must agree: the key is then the sequence followed by the feature's name without its
    variant. Prints what the reference prints, byte for byte; returns the number of inconsistent genomes (the reference
    returns None).

    df_features: LightSparseDataFrame or .npz path (stored entries, which must all be 1), pandas frame or csv / pickle path
    (a cell is present iff it == 1). Genomes are taken in sorted(genome_fasta_paths) order; a genome's column is the file's
    name without directory and extension or, if that is no column, that name without its last '_' piece (KeyError if
    neither is). The reference's quirks are kept: of two non-redundant records with one key the later header is the
    feature (and `COLLISION: <header>` is printed), `Missing Features:` is always 0, lines before the first '>' are a record
    named '', a record of blank lines is the sequence '', a header followed by a header is no record. When a genome's file
    is missing or is no column, what the genomes before it printed comes first, then its `Validating` line if due, then
    FileNotFoundError / KeyError.

    The reference compares SHA-256 digests of the keys; here the keys' bytes are compared, exactly, on the device
    (csrc/dict.hip: one dict_load of the non-redundant keys, one dict_query per batch of genomes bounded by
    TABLE_FASTA_BATCH_BYTES, one genome_sets_diff at the end). The two agree unless SHA-256 collides. The next genomes are
    parsed on a host thread while the device works. There is no CPU fallback."""
    import collections
    from concurrent.futures import ThreadPoolExecutor
    who = 'validate_table_against_fasta'
    rows, cols, labels, columns = _cells_equal_to_one(_load_table(df_features), who)
    if ctx is None:
        from . import _native
        ctx = _native.default_context()

    feature_to_allele = None
    if allele_names:
        print('Loading feature names...')
        feature_to_allele = _feature_to_allele(allele_names)

    print('Loading non-redundant sequences...')
    nr_headers, nr_keys = _fasta_records(features_fasta)
    if allele_names is not None:
        nr_keys = [seq + trim_variant(header).encode('utf-8') for header, seq in zip(nr_headers, nr_keys)]
    first = np.asarray(ctx.dict_load(*_blob(nr_keys)))
    repeated = np.flatnonzero(first != np.arange(first.size))
    for k in repeated.tolist():
        print('COLLISION:', nr_headers[k])
    print('Non-redundant sequences:', first.size - repeated.size)

    # names -> rows of the two bitmaps: a table label is its first row, then the non-redundant headers that are no label
    name_id = {}
    for r, label in enumerate(labels.tolist()):
        name_id.setdefault(label, r)
    n_names = labels.size
    name_of_key = np.empty(len(nr_headers), dtype=np.int32)
    for k, header in enumerate(nr_headers):
        at = name_id.get(header)
        if at is None:
            at = name_id[header] = n_names
            n_names += 1
        name_of_key[k] = at
    first_row = np.fromiter((name_id[label] for label in labels.tolist()), dtype=np.int32, count=labels.size)
    column_of = {}
    for j, label in enumerate(columns.tolist()):
        column_of.setdefault(label, j)
    order = np.argsort(cols, kind='stable')
    rows, cols = rows[order], cols[order]
    col_start = np.searchsorted(cols, np.arange(columns.size + 1))

    paths = sorted(genome_fasta_paths)
    suffix_of = {}
    genome_names = []                                     # of the genomes whose records were looked up
    a_rows, a_genomes, b_rows, b_genomes = [], [], [], []
    failure = None                                        # the exception the reference raises at genome len(genome_names)

    def flush(batch):
        """one dict_query for the records of the genomes in `batch`: (genome number, keys)"""
        keys = [key for _, genome_keys in batch for key in genome_keys]
        if not keys:
            return
        last = np.asarray(ctx.dict_query(*_blob(keys)))
        genome_of = np.repeat(np.array([g for g, _ in batch], dtype=np.int32),
                              np.array([len(k) for _, k in batch], dtype=np.int64))
        hit = last >= 0
        b_rows.append(name_of_key[last[hit]])
        b_genomes.append(genome_of[hit])

    with ThreadPoolExecutor(max_workers=1) as pool:
        pending = collections.deque()
        submitted = 0
        batch, batch_bytes = [], 0
        for g, path in enumerate(paths):
            while submitted < len(paths) and len(pending) < _TABLE_FASTA_AHEAD:
                pending.append(pool.submit(_genome_keys, paths[submitted], feature_to_allele, suffix_of))
                submitted += 1
            try:
                genome_keys = pending.popleft().result()
            except Exception as e:                        # re-raised below, after the lines of the genomes before this one
                failure = e
            if failure is None:
                genome = __get_genome_from_filename__(path)
                if genome not in column_of:
                    genome = '_'.join(genome.split('_')[:-1])
                if genome not in column_of:
                    failure = KeyError(genome)
            if failure is not None:
                for ahead in pending:
                    ahead.cancel()
                break
            genome_names.append(genome)
            j = column_of[genome]
            a_rows.append(first_row[rows[col_start[j]:col_start[j + 1]]])
            a_genomes.append(np.full(col_start[j + 1] - col_start[j], g, dtype=np.int32))
            n_bytes = sum(map(len, genome_keys))
            if batch and batch_bytes + n_bytes > TABLE_FASTA_BATCH_BYTES:
                flush(batch)
                batch, batch_bytes = [], 0
            batch.append((g, genome_keys))
            batch_bytes += n_bytes
        flush(batch)

    n_genomes = len(genome_names)
    if n_genomes:
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)      # noqa: E731
        table_only, genome_only = ctx.genome_sets_diff(cat(a_rows), cat(a_genomes), cat(b_rows), cat(b_genomes), n_names,
                                                       n_genomes)
    inconsistencies = 0
    for g in range(n_genomes + (failure is not None)):
        if (g + 1) % log_group == 0:
            print('Validating genome', g + 1, ':', paths[g])
        if g == n_genomes:
            raise failure
        if table_only[g] or genome_only[g]:
            inconsistencies += 1
            print(genome_names[g], '\t', 'Table only:', int(table_only[g]), '\t', 'Genome only:', int(genome_only[g]))
    print('Missing Features:', 0)                         # (the reference increments a copy, :1494-1512)
    print('Feature Table Inconsistencies:', inconsistencies)
    return inconsistencies


def validate_allele_table(df_alleles, genome_fasta_paths, alleles_fasta, log_group=1, ctx=None):
    """validate_table_against_fasta without allele names: an allele x genome table, CDS or non-coding, against the FAA / FNA
    files of the genomes and the non-redundant sequences (reference :1391-1415)."""
    return validate_table_against_fasta(df_alleles, genome_fasta_paths, alleles_fasta, None, log_group, ctx)


def validate_upstream_table(df_upstream, upstream_fna_paths, nr_upstream_fna, allele_names, log_group=1, ctx=None):
    """validate_table_against_fasta for an upstream x genome table and the extracted upstream sequences of every genome;
    allele_names tells conserved UTRs of different genes apart (reference :1333-1359)."""
    return validate_table_against_fasta(df_upstream, upstream_fna_paths, nr_upstream_fna, allele_names, log_group, ctx)


def validate_downstream_table(df_downstream, downstream_fna_paths, nr_downstream_fna, allele_names, log_group=1, ctx=None):
    """validate_table_against_fasta for a downstream x genome table (reference :1362-1388)."""
    return validate_table_against_fasta(df_downstream, downstream_fna_paths, nr_downstream_fna, allele_names, log_group, ctx)


# ---------------------------------------------------------------------------
# annotations (reference pangenome.py:1650-1810). Without ctx the two functions are the reference's loops, statement for
# statement, with urllib.unquote spelt urllib.parse.unquote (the reference raises AttributeError there on Python 3). With a
# _native.Context, extract_annotations matches protein ids against the GFF keys with the exact dictionary (csrc/dict.hip)
# and de-duplicates and votes on the device (csrc/annot.hip); generate_annotations is one dictionary load and
# one query. As for the proximal builders, only REGULAR input is handled: for anything else the device function returns
# None before it has written or printed anything and the host function runs, called exactly as without ctx.
# ---------------------------------------------------------------------------
ANNOTATION_PATH_COUNTS = collections.Counter()  # extract_device / extract_host / generate_device / generate_host per call
_DICT_MAX_KEYS, _DICT_MAX_BYTES, _ANNOT_MAX_TOKENS = 1 << 24, 1 << 32, 1 << 31   # the limits of pgx_dict_* and pgx_annot_vote


def _generate_annotations_host(features, annotation_files):
    import pandas as pd
    relevant_features = list(features) + []
    for feature in features:
        name, cluster_type, cluster_num, variant_type, variant_num = breakdown_feature_name(feature)
        if variant_type:                                     # variant-level feature
            relevant_features.append(name + '_' + cluster_type + str(cluster_num))
    relevant_features = set(relevant_features)
    relevant_annotations = {}
    for annot_file in annotation_files:
        with open(annot_file, 'r') as f:
            for line in f:
                data = line.strip().split('\t')
                feature = data[0]
                if feature in relevant_features:
                    relevant_annotations[feature] = ';'.join(data[1:])
    feature_to_annot = {}
    for feature in features:
        if feature in relevant_annotations:                  # direct annotation exists
            feature_to_annot[feature] = relevant_annotations[feature]
        else:                                                # possible cluster-level annotation exists
            name, cluster_type, cluster_num, variant_type, variant_num = breakdown_feature_name(feature)
            feature_cluster = name + '_' + cluster_type + str(cluster_num)
            if variant_type is not None and feature_cluster in relevant_annotations:
                feature_to_annot[feature] = relevant_annotations[feature_cluster]
            else:                                            # cluster-level annotation is missing
                feature_to_annot[feature] = np.nan
    return pd.Series(feature_to_annot, index=features)


def _extract_annotations_host(genome_gffs, allele_name_file, annotations_out, batch, collapse_alleles, flexible_locus_tag,
                              allowed_features):
    tmp_out = annotations_out + '.tmp'
    shutil.copyfile(allele_name_file, tmp_out)
    n_gffs = len(genome_gffs)
    for g in range(0, n_gffs, batch):
        annotations = {}
        for gff in genome_gffs[g:g + batch]:
            with open(gff, 'r') as f_gff:
                for line in f_gff:
                    data = line.strip().split('\t')
                    if len(data) == 9:
                        feature_type = data[2]
                        if allowed_features is None or feature_type in allowed_features:
                            line_annots = data[-1].split(';')
                            line_annots = dict(map(lambda x: x.split('='), line_annots))
                            if 'ID' in line_annots and 'product' in line_annots:
                                product = urllib.parse.unquote(line_annots['product'])   # replace % hex characters
                                fid2 = line_annots['ID']
                                fid3 = None
                                if 'locus_tag' in line_annots:
                                    fid3 = fid2 + '|' + line_annots['locus_tag']
                                if flexible_locus_tag:       # save both names when possible
                                    annotations[fid2] = product
                                    if fid3 is not None:
                                        annotations[fid3] = product
                                else:                        # save only 3-term, or only 2-term if no locus_tag
                                    annotations[fid2 if fid3 is None else fid3] = product
        print('Loaded', len(annotations), 'annotations from batch', g + 1, '-', min(n_gffs, g + batch))
        with open(tmp_out, 'r') as f_last:
            with open(tmp_out + '2', 'w+') as f_next:
                for line in f_last:
                    data = line.strip().split('\t')
                    allele, fids = data[0], data[1:]
                    fids = map(lambda x: annotations[x] if x in annotations else x, fids)
                    fids = list(collections.OrderedDict.fromkeys(fids))   # remove duplicate annotations
                    f_next.write(allele + '\t' + '\t'.join(fids) + '\n')
        shutil.move(tmp_out + '2', tmp_out)                  # remove last round
    if collapse_alleles:
        with open(tmp_out, 'r') as f_last:
            current_cluster = None
            with open(annotations_out, 'w+') as f_next:
                for line in f_last:
                    data = line.strip().split('\t')
                    allele = data[0]
                    cluster = __get_gene_from_allele__(allele)
                    allele_annots = '\t'.join(data[1:])
                    if current_cluster is None:              # initialize first cluster
                        current_cluster = cluster
                        cluster_alleles = [allele]
                        cluster_annots = [allele_annots]
                    elif cluster == current_cluster:         # continuing current cluster
                        cluster_alleles.append(allele)
                        cluster_annots.append(allele_annots)
                    else:                                    # start of new cluster: the last one of the file is never written
                        most_common_annot, count = collections.Counter(cluster_annots).most_common(1)[0]
                        f_next.write(current_cluster + '\t' + most_common_annot + '\n')
                        for i, annots in enumerate(cluster_annots):
                            if annots != most_common_annot:
                                f_next.write(cluster_alleles[i] + '\t' + annots + '\n')
                        current_cluster = cluster
                        cluster_alleles = [allele]
                        cluster_annots = [allele_annots]
        os.remove(tmp_out)
    else:
        shutil.move(tmp_out, annotations_out)


def _spans_blob(arr, starts, ends):
    """(blob uint8, offsets uint64) of the byte strings arr[starts[i]:ends[i]]"""
    lens = np.asarray(ends, dtype=np.int64) - np.asarray(starts, dtype=np.int64)
    offsets = np.zeros(lens.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    return arr[_ragged_index(starts, lens)], offsets


def _join_blobs(blobs):
    """several (blob, offsets) end to end"""
    blob = np.concatenate([b for b, _ in blobs]) if blobs else np.zeros(0, dtype=np.uint8)
    offsets, base = [np.zeros(1, dtype=np.uint64)], 0
    for b, off in blobs:
        offsets.append(off[1:] + np.uint64(base))
        base += int(off[-1])
    return blob, np.concatenate(offsets)


def _annotation_keys(g, flexible_locus_tag, allowed):
    """The records of one parsed GFF that extract_annotations stores, in file order: (key blob, key offsets, record of
    each key, product blob, product offsets), or None if a line is not regular."""
    if g['comment_records']:
        return None
    arr, n = g['arr'], g['n']
    (p_start, p_end), (l_start, l_end), (i_start, i_end) = g['product'], g['locus_tag'], g['id']
    take = p_start >= 0
    if allowed is not None and n:
        ty_start, ty_end = g['type']
        take &= np.isin(_fixed_width(arr, ty_start, ty_end - ty_start), allowed) if allowed.size else False
    rec = np.flatnonzero(take)
    has_tag = l_start[rec] >= 0
    # ID|locus_tag is ID, '|' and the tag: three pieces of the file's bytes with a '|' appended to them
    src = np.concatenate((arr, np.frombuffer(b'|', dtype=np.uint8)))
    bar = arr.size
    if flexible_locus_tag:
        kinds = [(rec, False), (rec[has_tag], True)]
    else:
        kinds = [(rec[~has_tag], False), (rec[has_tag], True)]
    owner = np.concatenate([r for r, _ in kinds])
    tagged = np.concatenate([np.full(r.size, t, dtype=bool) for r, t in kinds])
    order = np.argsort(owner, kind='stable')                 # file order; a record's two keys follow each other
    owner, tagged = owner[order], tagged[order]
    piece_start = np.stack((i_start[owner], np.full(owner.size, bar, dtype=np.int64), l_start[owner]), axis=1)
    piece_len = np.stack((i_end[owner] - i_start[owner], tagged.astype(np.int64),
                          np.where(tagged, l_end[owner] - l_start[owner], 0)), axis=1)
    piece_start = np.where(piece_len > 0, piece_start, 0)
    keys = src[_ragged_index(piece_start.reshape(-1), piece_len.reshape(-1))]
    key_off = np.zeros(owner.size + 1, dtype=np.uint64)
    np.cumsum(piece_len.sum(axis=1), out=key_off[1:])
    products, product_off = _spans_blob(arr, p_start[rec], p_end[rec])
    return keys, key_off, np.searchsorted(rec, owner), products, product_off


def _parse_names_regular(data):
    """The lines of an allele names file as arrays, or None if the file is not regular: arr, n, allele (start, end), gene_end
    (the last 'A' of the allele, its start for one without), fid (start, end of every protein id, line after line), n_fids."""
    if not data or not _plain_ascii(data) or data.translate(None, b' \x0b\x0c') != data:
        return None
    arr = np.frombuffer(data, dtype=np.uint8)
    ls, le = _line_spans(arr)
    if (le <= ls).any():
        return None                                          # a blank line: the allele '' with one empty id
    if (arr[ls] == 9).any() or (arr[le - 1] == 9).any():
        return None                                          # strip() would change the line
    tabs = np.flatnonzero(arr == 9)
    if tabs.size > 1 and (np.diff(tabs) == 1).any():
        return None                                          # an empty id
    lo = np.searchsorted(tabs, ls)
    n_fids = np.searchsorted(tabs, le) - lo
    a_end = np.where(n_fids > 0, tabs[np.minimum(lo, max(tabs.size - 1, 0))] if tabs.size else le, le)
    f_start = tabs + 1
    f_end = np.concatenate((tabs[1:], np.zeros(1, dtype=np.int64))) if tabs.size else tabs
    last_of_line = np.cumsum(n_fids) - 1
    f_end[last_of_line[n_fids > 0]] = le[n_fids > 0]
    big_a = np.flatnonzero(arr == 65)
    of_line = np.searchsorted(ls, big_a, side='right') - 1
    inside = big_a < a_end[of_line]
    gene_end = ls.copy()
    gene_end[of_line[inside]] = big_a[inside]                # ascending positions: the last one of a line stays
    return dict(arr=arr, n=ls.size, allele=(ls, a_end), gene_end=gene_end, fid=(f_start, f_end), n_fids=n_fids)


def _extract_annotations_device(ctx, genome_gffs, allele_name_file, annotations_out, batch, collapse_alleles,
                                flexible_locus_tag, allowed_features):
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        return None
    allowed = None
    if allowed_features is not None:
        if not isinstance(allowed_features, (list, tuple, set, frozenset)) or \
                not all(isinstance(x, str) for x in allowed_features):
            return None                                      # (`in` on a string is a substring test)
        allowed = np.array([x.encode('ascii') for x in allowed_features if x.isascii()], dtype='S')
    genome_gffs = list(genome_gffs)
    try:
        with open(allele_name_file, 'rb') as f:
            names = _parse_names_regular(f.read())
        if names is None:
            return None
        # the GFFs: batches in reverse, file order inside a batch, so that the largest index of a key is the record the
        # reference keeps -- the last one of the first batch that holds the key
        n_gffs = len(genome_gffs)
        batch_starts = list(range(0, n_gffs, batch))
        parts, batch_of_part = [], []
        for b in reversed(range(len(batch_starts))):
            for gff in genome_gffs[batch_starts[b]:batch_starts[b] + batch]:
                with open(gff, 'rb') as f:
                    g = _parse_gff_regular(f.read())
                part = None if g is None else _annotation_keys(g, flexible_locus_tag, allowed)
                if part is None:
                    return None
                parts.append(part)
                batch_of_part.append(b)
    except (OSError, TypeError, ValueError):
        return None
    keys, key_off = _join_blobs([(p[0], p[1]) for p in parts])
    products, product_off = _join_blobs([(p[3], p[4]) for p in parts])
    n_records = np.array([p[4].size - 1 for p in parts], dtype=np.int64)
    record_base = np.cumsum(n_records) - n_records
    record_of_key = np.concatenate([p[2] + base for p, base in zip(parts, record_base)]) if parts else np.zeros(0, np.int64)
    batch_of_key = np.repeat(np.array(batch_of_part, dtype=np.int64), [p[1].size - 1 for p in parts])
    f_start, f_end = names['fid']
    fids, fid_off = _spans_blob(names['arr'], f_start, f_end)
    n_keys, n_products, n_tokens = key_off.size - 1, product_off.size - 1, fid_off.size - 1
    if max(n_keys, n_products, n_tokens, names['n']) >= _DICT_MAX_KEYS or n_tokens >= _ANNOT_MAX_TOKENS or \
            max(int(key_off[-1]), int(product_off[-1]), int(fid_off[-1])) >= _DICT_MAX_BYTES:
        return None
    # the distinct raw products, decoded once each
    raw_first = ctx.dict_load(products, product_off)
    distinct_raw = np.flatnonzero(raw_first == np.arange(n_products))
    decoded, decoded_id = [], {}
    text_of_raw = np.zeros(n_products, dtype=np.int64)
    raw_bytes = products.tobytes()
    for r in distinct_raw.tolist():
        text = urllib.parse.unquote(raw_bytes[int(product_off[r]):int(product_off[r + 1])].decode('ascii'))
        if not text or not text.isascii() or text.strip() != text or '\t' in text or '\n' in text or '\r' in text:
            return None
        text_of_raw[r] = decoded_id.setdefault(text, len(decoded))
        if text_of_raw[r] == len(decoded):
            decoded.append(text.encode('ascii'))
    text_of_record = text_of_raw[raw_first]
    decoded_blob, decoded_off = _blob(decoded)
    # the keys; a product that is itself a key would be replaced again by a later batch: the host knows how
    key_first = ctx.dict_load(keys, key_off)
    if decoded and (ctx.dict_query(decoded_blob, decoded_off) >= 0).any():
        return None
    last = ctx.dict_query(fids, fid_off)
    loaded = np.bincount(np.unique(batch_of_key * _DICT_MAX_KEYS + key_first) // _DICT_MAX_KEYS, minlength=len(batch_starts))
    # one id space for products and the ids nothing replaced: the first of the equal strings
    mapped = last >= 0
    loose = np.flatnonzero(~mapped)
    loose_blob, loose_off = _spans_blob(names['arr'], f_start[loose], f_end[loose])
    text_blob, text_off = _join_blobs([(decoded_blob, decoded_off), (loose_blob, loose_off)])
    if text_off.size - 1 >= _DICT_MAX_KEYS or int(text_off[-1]) >= _DICT_MAX_BYTES:
        return None
    text_first = ctx.dict_load(text_blob, text_off)
    tok = np.zeros(n_tokens, dtype=np.int32)
    tok[mapped] = text_first[text_of_record[record_of_key[last[mapped]]]]
    tok[loose] = text_first[len(decoded) + np.arange(loose.size)]
    n_fids = names['n_fids']
    row_off = np.zeros(names['n'] + 1, dtype=np.uint64)
    np.cumsum(n_fids, out=row_off[1:])
    a_start, a_end = names['allele']
    if collapse_alleles:
        genes = _fixed_width(names['arr'], a_start, names['gene_end'] - a_start)
        run_start = np.flatnonzero(np.concatenate((np.ones(1, dtype=bool), genes[1:] != genes[:-1])))
    else:
        run_start = np.arange(names['n'])
    run_off = np.concatenate((run_start, [names['n']])).astype(np.uint32)
    keep, winner, votes, differs = ctx.annot_vote(tok, row_off, run_off)
    # the output, one gather: a line is a name, '\t' + text per kept id ('\t' alone for none), '\n'
    n_runs = run_off.size - 1
    if collapse_alleles:
        # per run but the last: the gene with the winner's list, then the alleles that differ
        closed = np.arange(names['n']) < int(run_off[n_runs - 1])
        odd = np.flatnonzero((differs != 0) & closed)
        heads = np.arange(n_runs - 1)
        line_run = np.concatenate((heads, np.searchsorted(run_off, odd, side='right') - 1))
        order = np.argsort(line_run, kind='stable')          # a run's gene line first, its alleles in file order
        row = np.concatenate((winner[:n_runs - 1].astype(np.int64), odd))[order]
        name_start = np.concatenate((a_start[run_off[:n_runs - 1].astype(np.int64)], a_start[odd]))[order]
        name_end = np.concatenate((names['gene_end'][run_off[:n_runs - 1].astype(np.int64)], a_end[odd]))[order]
    else:
        row = np.arange(names['n'], dtype=np.int64)
        name_start, name_end = a_start, a_end
    kept_pos = np.flatnonzero(keep != 0)
    kept_off = np.searchsorted(kept_pos, row_off.astype(np.int64))          # kept ids before each row
    k = kept_off[row + 1] - kept_off[row]
    line_tok = tok[kept_pos[_ragged_index(kept_off[row], k)]]
    # the source: the names file, then '\t' + text of every string, then '\t\n'
    tab = np.frombuffer(b'\t', dtype=np.uint8)
    text_len = np.diff(text_off.astype(np.int64))
    tabbed_off = text_off.astype(np.int64) + np.arange(text_off.size)
    tabbed = np.zeros(int(tabbed_off[-1]), dtype=np.uint8)
    tabbed[tabbed_off[:-1]] = 9
    tabbed[_ragged_index(tabbed_off[:-1] + 1, text_len)] = text_blob
    base_text = names['arr'].size
    base_end = base_text + tabbed.size
    src = np.concatenate((names['arr'], tabbed, tab, np.frombuffer(b'\n', dtype=np.uint8)))
    pieces_off = np.cumsum(k + 2) - (k + 2)
    n_pieces = int((k + 2).sum())
    p_start, p_len = np.zeros(n_pieces, dtype=np.int64), np.zeros(n_pieces, dtype=np.int64)
    is_token = np.ones(n_pieces, dtype=bool)
    p_start[pieces_off], p_len[pieces_off] = name_start, name_end - name_start
    ends = pieces_off + k + 1
    p_start[ends], p_len[ends] = np.where(k > 0, base_end + 1, base_end), np.where(k > 0, 1, 2)
    is_token[pieces_off] = False
    is_token[ends] = False
    p_start[is_token], p_len[is_token] = base_text + tabbed_off[line_tok], text_len[line_tok] + 1
    out = src[_ragged_index(p_start, p_len)]
    for b, g in enumerate(batch_starts):
        print('Loaded', int(loaded[b]), 'annotations from batch', g + 1, '-', min(n_gffs, g + batch))
    with open(annotations_out, 'wb') as f:
        f.write(out.tobytes())
    for stale in (annotations_out + '.tmp', annotations_out + '.tmp2'):
        if os.path.exists(stale):
            os.remove(stale)
    return True


def extract_annotations(genome_gffs, allele_name_file, annotations_out, batch=100, collapse_alleles=True,
                        flexible_locus_tag=False, allowed_features=None, ctx=None):
    """For an allele names file (usually <name>_allele_names.tsv), replaces every protein id by the product of its GFF
    record (key ID|locus_tag, or ID without a tag; both with flexible_locus_tag), drops repeats, and with collapse_alleles
    writes per gene the most common annotation of its alleles followed by the alleles that differ (reference :1702-1810,
    quirks included: the last gene of the file is never written). ctx: a _native.Context for the device path."""
    if ctx is not None and _extract_annotations_device(ctx, genome_gffs, allele_name_file, annotations_out, batch,
                                                       collapse_alleles, flexible_locus_tag, allowed_features):
        ANNOTATION_PATH_COUNTS['extract_device'] += 1
        return
    ANNOTATION_PATH_COUNTS['extract_host'] += 1
    _extract_annotations_host(genome_gffs, allele_name_file, annotations_out, batch, collapse_alleles, flexible_locus_tag,
                              allowed_features)


def _generate_annotations_device(ctx, features, annotation_files):
    import pandas as pd
    index = features
    try:
        features = list(features)
        clusters = []
        for feature in features:
            name, cluster_type, cluster_num, variant_type, variant_num = breakdown_feature_name(feature)
            clusters.append(name + '_' + cluster_type + str(cluster_num) if variant_type else None)
        if not all(isinstance(x, str) and x.isascii() for x in features):
            return None
        datas = []
        for annot_file in annotation_files:
            with open(annot_file, 'rb') as f:
                datas.append(f.read())
    except Exception:                                        # (the host function raises it again, in its own order)
        return None
    data = b''.join(datas)
    if any(d and not d.endswith(b'\n') for d in datas[:-1]) or not _plain_ascii(data):
        return None
    arr = np.frombuffer(data, dtype=np.uint8)
    ls, le = _line_spans(arr)
    if ls.size and ((le <= ls).any() or _PROX_SPACE[arr[ls]].any() or _PROX_SPACE[arr[np.maximum(le, 1) - 1]].any()):
        return None                                          # strip() would change a line
    tabs = np.flatnonzero(arr == 9)
    lo = np.searchsorted(tabs, ls)
    has_tab = np.searchsorted(tabs, le) > lo
    name_end = np.where(has_tab, tabs[np.minimum(lo, tabs.size - 1)], le) if tabs.size else le
    keys, key_off = _spans_blob(arr, ls, name_end)
    queries = features + [c for c in clusters if c is not None]
    q_blob, q_off = _blob([q.encode('ascii') for q in queries])
    if max(key_off.size, q_off.size) - 1 >= _DICT_MAX_KEYS or max(int(key_off[-1]), int(q_off[-1])) >= _DICT_MAX_BYTES:
        return None
    ctx.dict_load(keys, key_off, want_first=False)           # later line = larger index: last[] is the line that stays
    last = ctx.dict_query(q_blob, q_off)
    own = last[:len(features)]
    of_cluster = np.full(len(features), -1, dtype=np.int64)
    of_cluster[[i for i, c in enumerate(clusters) if c is not None]] = last[len(features):]
    line = np.where(own >= 0, own, of_cluster)
    text = {int(i): ';'.join(data[int(name_end[i]) + 1:int(le[i])].decode('ascii').split('\t')) if has_tab[i] else ''
            for i in np.unique(line[line >= 0])}
    feature_to_annot = {feature: (text[int(i)] if i >= 0 else np.nan) for feature, i in zip(features, line.tolist())}
    return pd.Series(feature_to_annot, index=index)


def generate_annotations(features, annotation_files, ctx=None):
    """A pd.Series of annotations indexed by `features`, from files extract_annotations wrote: a feature's own line, else
    for a variant the line of its cluster <name>_<type><num>, else np.nan; a later line or file replaces an earlier one
    (reference :1650-1699). ctx: a _native.Context for the device path."""
    if ctx is not None:
        series = _generate_annotations_device(ctx, features, annotation_files)
        if series is not None:
            ANNOTATION_PATH_COUNTS['generate_device'] += 1
            return series
    ANNOTATION_PATH_COUNTS['generate_host'] += 1
    return _generate_annotations_host(features, annotation_files)
