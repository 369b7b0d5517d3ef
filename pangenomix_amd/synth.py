"""Deterministic synthetic inputs for tests and bench.py (SURVEY.md §8d recipe; the
Bacteroides .faa sets the reference was used on are not available offline).

Protein set: F family ancestors with lengths clip(gamma(2.2, 150), 40, 2500) over the 20
standard letters; each genome holds C core families plus accessory families drawn without
replacement; an instance copies its ancestor, with prob. 0.6 substitutes 2 % of its sites,
a 5 % tier substitutes 15-25 % (straddles the 0.8 threshold), and 1 % of the records are
<= 10 residues long (exercises cd-hit's discard length).
"""

import collections
import os
import sys

import numpy as np

AA20 = np.frombuffer(b'ACDEFGHIKLMNPQRSTVWY', dtype=np.uint8)

CONFIGS = {
    # name: (genomes, cds/genome, families, core families, seed)
    'tiny': (6, 60, 150, 30, 6),
    'small': (20, 400, 1500, 200, 20),
    'cfg-2s': (50, 4500, 30000, 2000, 50),
    'cfg-3s': (400, 4500, 30000, 2000, 400),
    'cfg-4': (4000, 3000, 60000, 1500, 4000),
}


class ProteinSet(object):
    def __init__(self, n_genomes, cds_per_genome, n_families, n_core, seed):
        self.n_genomes, self.cds, self.F, self.C, self.seed = n_genomes, cds_per_genome, n_families, n_core, seed
        rng = np.random.default_rng(seed)
        lens = np.clip(rng.gamma(2.2, 150.0, n_families), 40, 2500).astype(np.int64)
        self.fam_off = np.zeros(n_families + 1, dtype=np.int64)
        np.cumsum(lens, out=self.fam_off[1:])
        self.fam_res = AA20[rng.integers(0, 20, int(self.fam_off[-1]))]
        self.fam_len = lens

    def genome(self, g):
        """(family ids, [bytes sequence per record]) of genome g; deterministic in (seed, g)."""
        rng = np.random.default_rng([self.seed, g])
        n_acc = self.cds - self.C
        acc = self.C + rng.choice(self.F - self.C, size=n_acc, replace=False)
        fams = np.concatenate([np.arange(self.C), acc])
        rng.shuffle(fams)
        tier = rng.random(fams.size)
        seqs = []
        for k, f in enumerate(fams):
            s = self.fam_res[self.fam_off[f]:self.fam_off[f + 1]].copy()
            t = tier[k]
            if t < 0.01:                       # too short for cd-hit
                s = s[:int(rng.integers(3, 11))]
            elif t < 0.06:                     # 15-25 % substituted
                self._mutate(rng, s, rng.uniform(0.15, 0.25))
            elif t < 0.06 + 0.94 * 0.6:        # 2 % substituted
                self._mutate(rng, s, 0.02)
            seqs.append(s.tobytes())
        return fams, seqs

    @staticmethod
    def _mutate(rng, s, frac):
        n = max(1, int(round(frac * s.size)))
        pos = rng.choice(s.size, size=n, replace=False)
        s[pos] = AA20[rng.integers(0, 20, n)]

    def header(self, g, k, fam):
        return 'fig|%d.1.peg.%d|F%d' % (g, k, fam)

    def write_faa(self, directory, wrap=60):
        """One <directory>/genome_<g>.faa per genome; returns the paths."""
        os.makedirs(directory, exist_ok=True)
        paths = []
        for g in range(self.n_genomes):
            fams, seqs = self.genome(g)
            path = os.path.join(directory, 'genome_%04d.faa' % g)
            with open(path, 'w') as f:
                for k, (fam, s) in enumerate(zip(fams, seqs)):
                    s = s.decode('ascii')
                    f.write('>%s   hypothetical protein\n' % self.header(g, k, fam))
                    f.write('\n'.join(s[i:i + wrap] for i in range(0, len(s), wrap)) + '\n')
            paths.append(path)
        return paths

    def nr_arrays(self, progress=None):
        """Exact-deduplicated records in genome order (what consolidate_seqs hands to the
        clustering call): (residues uint8 ASCII, offsets uint64, n_raw)."""
        seen, chunks, lens, n_raw = set(), [], [], 0
        for g in range(self.n_genomes):
            _, seqs = self.genome(g)
            n_raw += len(seqs)
            for s in seqs:
                if s not in seen:
                    seen.add(s)
                    chunks.append(s)
                    lens.append(len(s))
            if progress and (g + 1) % progress == 0:
                print('  synth: genome %d / %d, %d non-redundant' % (g + 1, self.n_genomes, len(lens)), file=sys.stderr, flush=True)
        offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
        np.cumsum(np.asarray(lens, dtype=np.uint64), out=offsets[1:])
        residues = np.frombuffer(b''.join(chunks), dtype=np.uint8)
        return residues, offsets, n_raw


def protein_set(name):
    return ProteinSet(*CONFIGS[name])


def pancore_matrix(n_genes=150000, n_genomes=400, seed=1):
    """Synthetic gene x genome presence matrix of SURVEY §8d: 2,000 genes at p=0.99, the rest
    Beta(0.08, 3); rows that come out empty are dropped and drawing continues until exactly
    `n_genes` non-empty rows exist. Returns COO (row int32, col int32, n_genes)."""
    rng = np.random.default_rng(seed)
    rows, cols, have = [], [], 0
    first = True
    while have < n_genes:
        chunk = 20000
        p = rng.beta(0.08, 3.0, chunk)
        if first:
            p[:min(2000, chunk)] = 0.99
            first = False
        m = rng.random((chunk, n_genomes)) < p[:, None]
        m = m[m.any(axis=1)][:n_genes - have]
        r, c = np.nonzero(m)
        rows.append(r + have)
        cols.append(c)
        have += m.shape[0]
    return (np.concatenate(rows).astype(np.int32), np.concatenate(cols).astype(np.int32), int(n_genes))


def _revcomp(b):
    return b[::-1].translate(bytes.maketrans(b'ACGT', b'TGCA'))


def noncoding_set(n_genomes=400, seed=5, n_trna=60, rrna_lengths=(120, 1500, 2900), copies_rrna=3):
    """Synthetic non-coding feature set of SURVEY §8d (config 5): per genome ~90 features --
    tRNA-like families (74-90 nt) and rRNA-like ones (120 / 1,500 / 2,900 nt) -- each copy
    0-10 % diverged from its ancestor, about half of them given on the reverse strand, a few
    with N. Returns the exact-deduplicated (residues uint8 ASCII, offsets uint64, n_raw)."""
    rng = np.random.default_rng(seed)
    nt = np.frombuffer(b'ACGT', dtype=np.uint8)
    fams = [nt[rng.integers(0, 4, int(rng.integers(74, 91)))] for _ in range(n_trna)]
    fams += [nt[rng.integers(0, 4, L)] for L in rrna_lengths for _ in range(copies_rrna)]
    seen, chunks, lens, n_raw = set(), [], [], 0
    for g in range(n_genomes):
        for f, anc in enumerate(fams):
            copies = 1 if f < n_trna else int(rng.integers(1, 4))
            for _ in range(copies):
                s = anc.copy()
                div = rng.uniform(0.0, 0.10) if rng.random() < 0.7 else 0.0
                k = int(div * s.size)
                if k:
                    pos = rng.choice(s.size, size=k, replace=False)
                    s[pos] = nt[rng.integers(0, 4, k)]
                if rng.random() < 0.02:
                    s[int(rng.integers(0, s.size))] = ord('N')
                b = s.tobytes()
                if rng.random() < 0.5:
                    b = _revcomp(b)
                n_raw += 1
                if b not in seen:
                    seen.add(b)
                    chunks.append(b)
                    lens.append(len(b))
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(lens, dtype=np.uint64), out=offsets[1:])
    return np.frombuffer(b''.join(chunks), dtype=np.uint8), offsets, n_raw


AMR_CLASS_NAMES = ('beta-lactam antibiotic', 'penam', 'monobactam', 'cephalosporin', 'carbapenem', 'aminoglycoside antibiotic',
                   'fluoroquinolone antibiotic', 'lincosamide antibiotic', 'macrolide antibiotic', 'phenicol antibiotic',
                   'nitrofuran antibiotic', 'tetracycline antibiotic', 'glycylcycline', 'diaminopyrimidine antibiotic',
                   'sulfonamide antibiotic', 'glycopeptide antibiotic')


def write_amr_case(outdir, class_aros, n_terms=300, n_hits=200, n_drugs=12, n_lines=2000, n_products=150, seed=0, name_every=3):
    """Inputs of pangenomix_amd.amr in `outdir`: aro.obo -- ARO:1000001, ARO:1000003 with the sixteen drug classes
    (`class_aros`, amr.DRUG_CLASS_AROS) and a tree of n_terms / 3 drugs and mixtures under them, n_terms * 2 / 3 resistance
    determinants in families, some of which confer resistance to a drug or a class, are part of or regulate another --,
    rgi.txt with n_hits rows (a few Loose, a few ORF_IDs twice) and annotations.tsv with n_lines lines of one to three of
    n_products products, every name_every-th of which names a drug, a part of a mixture or a class, in mixed case, and every
    seventh a class and a drug. Returns a dict: the three paths, `drugs`
    ({name: ARO} of n_drugs drugs, every fourth a mixture keyed 'a/b'), `drug_to_aro` and `manual_annots`."""
    rng = np.random.default_rng(seed)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]                      # noqa: E731
    blocks, drug_tree, drug_names, mixtures, genes = [], list(class_aros), {}, [], ['ARO:3000000']

    def term(aro, name, is_a, relationships=()):
        blocks.append('[Term]\nid: %s\nname: %s\n' % (aro, name) + ''.join('is_a: %s ! x\n' % p for p in is_a) +
                      ''.join('relationship: %s %s ! x\n' % r for r in relationships))
    term('ARO:1000001', 'process or component of antibiotic biology or chemistry', [])
    term('ARO:1000003', 'antibiotic molecule', ['ARO:1000001'])
    term('ARO:3000000', 'determinant of antibiotic resistance', ['ARO:1000001'])
    for aro, name in zip(class_aros, AMR_CLASS_NAMES):
        term(aro, name, ['ARO:1000003'])
    n_drug_terms = max(n_drugs + 4, n_terms // 3)
    for i in range(n_drug_terms):
        aro = 'ARO:%07d' % (4000000 + i)
        if i % 9 == 8 and len(drug_names) >= 2:                                 # a mixture of two drugs
            a, b = pick(list(drug_names)), pick(list(drug_names))
            term(aro, 'mix%d' % i, ['ARO:1000003'], [('has_part', a), ('has_part', b)])
            mixtures.append((aro, drug_names[a] + '/' + drug_names[b]))
        else:
            term(aro, 'drug%03dicin' % i, [pick(drug_tree)])
            drug_tree.append(aro)
            drug_names[aro] = 'drug%03dicin' % i
    drugs = {}
    singles = list(drug_names.items())
    for k in range(n_drugs):
        if k % 4 == 3 and mixtures:
            aro, name = mixtures[k // 4 % len(mixtures)]
        else:
            aro, name = singles[int(rng.integers(0, len(singles)))]
        drugs[name] = aro
    of_interest = [aro for aro in drugs.values() if aro in drug_names] or list(drug_names)
    families = []
    for i in range(n_terms - n_drug_terms):
        aro = 'ARO:%07d' % (5000000 + i)
        rel = []
        if rng.random() < 0.08:                                                 # half of them to a drug of interest
            rel.append(('confers_resistance_to_antibiotic', pick(of_interest if rng.random() < 0.5 else list(drug_names))))
        if rng.random() < 0.03:
            rel.append(('confers_resistance_to_drug_class', pick(list(class_aros))))
        if rng.random() < 0.05:
            rel.append((pick(['part_of', 'regulates', 'participates_in']), pick(genes)))
        if not families or rng.random() < 0.08:                                 # a new family, or a member of a recent one
            parent = 'ARO:3000000'
            families.append([aro])
        else:
            family = families[int(rng.integers(max(0, len(families) - 10), len(families)))]
            parent = pick(family)
            family.append(aro)
        term(aro, 'det%d' % i, [parent], rel)
        genes.append(aro)
    with open(os.path.join(outdir, 'aro.obo'), 'w') as f:
        f.write('format-version: 1.2\n\n' + '\n'.join(blocks) + '\n[Typedef]\nid: part_of\n')

    drug_list = list(drugs)
    with open(os.path.join(outdir, 'rgi.txt'), 'w') as f:
        f.write('ORF_ID\tCut_Off\tBest_Hit_ARO\tARO\n')
        for h in range(n_hits):
            orf = 'Syn_C%dA%d' % (h // 3 if h % 17 else max(h // 3 - 2, 0), h % 3)   # every 17th: an earlier ORF_ID again
            gene = pick(genes[1:])
            f.write('%s\t%s\tdet\t%d\n' % (orf, 'Loose' if h % 11 == 5 else pick(['Strict', 'Perfect']), int(gene[4:])))
    words = ['protein', 'Resistance', 'efflux pump', 'hydrolase', 'transporter', 'family', 'regulator', 'subunit A', 'kinase']
    products = ['hypothetical protein']
    for p in range(n_products - 1):
        parts = [pick(words), pick(words)]
        if p % name_every == 0:                                                 # names a drug of interest, a part, a class
            drug = pick(drug_list)
            parts.insert(1, pick([drug, drug.split('/')[0].upper(), pick(AMR_CLASS_NAMES).replace(' antibiotic', '').title()]))
        if p % 7 == 0:
            parts.append(pick(AMR_CLASS_NAMES).split()[0] + ' ' + pick(drug_list).split('/')[-1])
        products.append(' '.join(parts) + ' %d' % p)
    with open(os.path.join(outdir, 'annotations.tsv'), 'w') as f:
        for i in range(n_lines):
            feature = 'Syn_C%dA%d' % (i // 3, i % 3) if i % 5 else 'Syn_C%d' % (i // 3)
            pool = products[:max(8, n_products // 10)] if i < n_hits else products   # the hits share a tenth of the products
            f.write('\t'.join([feature] + [pick(pool) for _ in range(int(rng.integers(1, 4)))]) + '\n')
    return {'obo': os.path.join(outdir, 'aro.obo'), 'rgi': os.path.join(outdir, 'rgi.txt'),
            'annotations': os.path.join(outdir, 'annotations.tsv'), 'drugs': drugs,
            'drug_to_aro': {drug_list[0]: genes[1]}, 'manual_annots': {drug_list[-1]: ['efflux pump', 'Kinase']}}


PATRIC_AMR_COLUMNS = ('genome_id', 'genome_name', 'taxon_id', 'antibiotic', 'resistant_phenotype', 'measurement',
                      'measurement_sign', 'measurement_value', 'measurement_unit', 'laboratory_typing_method',
                      'laboratory_typing_method_version', 'laboratory_typing_platform', 'vendor', 'testing_standard',
                      'testing_standard_year', 'computational_method', 'computational_method_version', 'source')


def patric_amr_table(n_rows=1000000, n_orgs=8, genomes_per_org=2000, n_drugs=40, seed=11):
    """(org_to_gids, df_amr): a table in the layout of PATRIC_genomes_AMR.txt for amr_inference, rows grouped by genome as
    in the real file. `measurement` carries an inequality and `measurement_value` does not; both are strings, so that a
    combination's 'a/b' stays what it is. Every organism x drug case has a susceptible and a resistant breakpoint on the
    two-fold dilution series; a MIC at either end of the series is reported as '<=' or '>'; a tenth of the rows has a
    phenotype and no measurement, a tenth a disk diffusion in mm; standards are clsi, eucast, 'missing' or null with
    weights that differ by organism. A twentieth of the genomes belongs to no organism. Nulls of object columns are the
    np.nan object, as pandas.read_csv leaves them."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    n_genomes = n_orgs * genomes_per_org
    orgs = ['Genus%02d species%02d' % (o, o) for o in range(n_orgs)]
    gids = np.array(['%d.%d' % (1000 + g // genomes_per_org, g % genomes_per_org) for g in range(n_genomes)], dtype=object)
    owned = rng.random(n_genomes) >= 0.05
    org_to_gids = {org: gids[o * genomes_per_org:(o + 1) * genomes_per_org][owned[o * genomes_per_org:(o + 1) * genomes_per_org]].tolist()
                   for o, org in enumerate(orgs)}
    drugs = np.array(['drug%02d' % d if d % 5 else 'drug%02d_partner%02d' % (d, d) for d in range(n_drugs)], dtype=object)
    drugs[1], drugs[2] = 'polymyxin_b', 'nalidixic_acid'
    is_combo = np.array([d % 5 == 0 for d in range(n_drugs)])
    series = 2.0 ** np.arange(-6, 9)                                         # 0.015625 .. 256
    text = np.array(['%g' % m for m in series], dtype=object)
    pair = np.array(['%g/%g' % (m, m / 2) for m in series], dtype=object)

    genome = np.sort(rng.integers(0, n_genomes, n_rows))
    org = genome // genomes_per_org
    # drugs are tested unevenly: some cases stay under min_entries
    weight = 1.0 / (1 + np.arange(n_drugs)) ** 0.7
    drug = rng.choice(n_drugs, n_rows, p=weight / weight.sum())
    s_break = rng.integers(4, 8, (n_orgs, n_drugs))                          # index of the largest susceptible MIC
    r_break = s_break + rng.integers(1, 3, (n_orgs, n_drugs))                # index of the smallest resistant MIC
    resistant = rng.random(n_rows) < rng.random((n_orgs, n_drugs))[org, drug]
    centre = np.where(resistant, r_break[org, drug] + 2, s_break[org, drug] - 2)
    mic = np.clip(centre + np.rint(rng.normal(0, 1.6, n_rows)).astype(np.int64), 0, series.size - 1)
    sir = np.where(mic <= s_break[org, drug], 0, np.where(mic >= r_break[org, drug], 1, 2))
    sir = np.where(rng.random(n_rows) < 0.01, rng.integers(0, 3, n_rows), sir)      # a few calls disagree
    sign = np.where(mic == 0, 3, np.where(mic == series.size - 1, 4, rng.choice(3, n_rows, p=[0.8, 0.15, 0.05])))
    signs = np.array([np.nan, '=', '==', '<=', '>'], dtype=object)
    prefix = np.array(['', '', '', '<=', '>'], dtype=object)
    value = np.where(is_combo[drug], pair[mic], text[mic]).astype(object)
    measurement = (prefix[sign] + value).astype(object)

    kind = rng.choice(3, n_rows, p=[0.8, 0.1, 0.1])                          # a MIC, a disk diffusion, a phenotype alone
    nothing = np.full(n_rows, np.nan, dtype=object)
    by_kind = lambda mic_rows, disk_rows: np.where(kind == 0, mic_rows, np.where(kind == 1, disk_rows, nothing))   # noqa: E731
    disk = np.array(['%d' % d for d in range(6, 40)], dtype=object)[rng.integers(0, 34, n_rows)]
    value, measurement = by_kind(value, disk), by_kind(measurement, disk)
    sign_col = by_kind(signs[sign], nothing)
    unit = np.array(['mg/L', 'mm', np.nan], dtype=object)[kind]
    methods = np.array(['broth_microdilution', 'etest', 'vitek_2', 'agar_dilution', 'sensititre', 'computational prediction'],
                       dtype=object)
    method = by_kind(methods[rng.choice(6, n_rows, p=[0.5, 0.15, 0.15, 0.1, 0.05, 0.05])],
                     np.full(n_rows, 'disk_diffusion', dtype=object))
    stnd_weight = rng.dirichlet([4, 2, 0.5, 1], n_orgs)
    stnd = np.array(['clsi', 'eucast', 'missing', np.nan], dtype=object)[
        (rng.random(n_rows)[:, None] > np.cumsum(stnd_weight, axis=1)[org]).sum(axis=1).clip(0, 3)]
    for col in (value, measurement, sign_col, unit, method, stnd):           # one null object, whatever np.where made
        col[pd.isnull(col)] = np.nan
    df = pd.DataFrame({
        'genome_id': gids[genome], 'genome_name': np.array(orgs, dtype=object)[org], 'taxon_id': 1000 + org, 'antibiotic': drugs[drug],
        'resistant_phenotype': np.array(['susceptible', 'resistant', 'intermediate'], dtype=object)[sir], 'measurement': measurement,
        'measurement_sign': sign_col, 'measurement_value': value, 'measurement_unit': unit, 'laboratory_typing_method': method,
        'laboratory_typing_method_version': nothing, 'laboratory_typing_platform': nothing, 'vendor': nothing,
        'testing_standard': stnd, 'testing_standard_year': np.where(pd.isnull(stnd), np.nan, 2015.0).astype(np.float64),
        'computational_method': nothing, 'computational_method_version': nothing,
        'source': np.full(n_rows, 'synthetic', dtype=object)}, columns=list(PATRIC_AMR_COLUMNS))
    return org_to_gids, df


def phylogeny(n_species, seed, n_genes=100, max_children=4, mapped_internal=0, unmapped_leaves=0, unused_species=0):
    """(G, root, mrca_to_species, df_genes_pa) for weboflife: a random rooted tree over n_species species as a
    weboflife.PhyloGraph with branch lengths in the edge attribute 'len', and a matching gene x species
    LightSparseDataFrame of ones. The tree is joined from the leaves up: two random subtrees at a time, three to
    max_children in three joins out of ten (polytomies), so its height grows like the logarithm of n_species and a little
    faster. Leaf 'L<i>' maps to species 'S<i>'; mapped_internal internal nodes (never the root) are mapped as well, each to
    the species of a random leaf, so that two nodes share it; unmapped_leaves childless nodes 'U<i>' hang below random
    internal nodes and map to nothing; unused_species further columns 'X<i>' are mapped by no node. A gene's frequency is
    drawn from a U-shaped distribution (most genes rare, some in nearly every species)."""
    import scipy.sparse as sp
    from . import sparse_utils, weboflife
    rng = np.random.default_rng(seed)
    pool = ['L%d' % i for i in range(n_species)]
    joins = []                                                                  # (parent, children), leaves first
    while len(pool) > 1:
        k = 2 if rng.random() < 0.7 or max_children < 3 else int(rng.integers(3, max_children + 1))
        children = []
        for _ in range(min(k, len(pool))):
            at = int(rng.integers(0, len(pool)))
            pool[at], pool[-1] = pool[-1], pool[at]
            children.append(pool.pop())
        parent = 'N%d' % len(joins)
        joins.append((parent, children))
        pool.append(parent)
    root = pool[0]
    extra = collections.defaultdict(list)
    if joins:
        for i, at in enumerate(rng.integers(0, len(joins), unmapped_leaves).tolist()):
            extra[joins[at][0]].append('U%d' % i)
    G = weboflife.PhyloGraph()
    G.add_node(root)
    for parent, children in reversed(joins):                                    # from the root down
        for child in children + extra[parent]:
            G.add_edge(parent, child, len=round(float(rng.uniform(0.01, 1.0)), 6))
    mrca_to_species = {'L%d' % i: 'S%d' % i for i in range(n_species)}
    inner = [parent for parent, _ in joins[:-1]]
    for at in rng.permutation(len(inner))[:mapped_internal].tolist():
        mrca_to_species[inner[at]] = 'S%d' % int(rng.integers(0, n_species))
    n_columns = n_species + unused_species
    frequency = rng.beta(0.25, 0.9, n_genes)
    rows, cols = [], []
    for lo in range(0, n_genes, 1024):                                          # (in slabs: the dense draw is the large part)
        hit = rng.random((min(1024, n_genes - lo), n_columns), dtype=np.float32) < frequency[lo:lo + 1024, None]
        r, c = np.nonzero(hit)
        rows.append((r + lo).astype(np.int32))
        cols.append(c.astype(np.int32))
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int32)
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int32)
    data = sp.coo_matrix((np.ones(rows.size, dtype=np.int8), (rows, cols)), shape=(n_genes, n_columns))
    index = np.array(['G%d' % g for g in range(n_genes)], dtype=object)
    columns = np.array(['S%d' % s for s in range(n_species)] + ['X%d' % s for s in range(unused_species)], dtype=object)
    return G, root, mrca_to_species, sparse_utils.LightSparseDataFrame(index, columns, data)


def mlst_scheme(n_loci=7, n_alleles=300, length=450, seed=21, max_mutations=3):
    """A synthetic typing scheme (pangenomix_amd.mlst.Scheme): n_loci loci of n_alleles distinct alleles of `length` bases,
    numbered from 1. The alleles of a locus are point mutants of one ancestor (1..max_mutations substitutions anywhere), so
    most of them share their first 32 bases and long stretches behind them. 50 profiles of random alleles, ST 1..50."""
    from . import mlst
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)
    loci = ['loc%c' % (ord('A') + i) if n_loci <= 26 else 'loc%d' % i for i in range(n_loci)]
    alleles = {}
    for locus in loci:
        ancestor = letters[rng.integers(0, 4, length)]
        seen, records = set(), []
        while len(records) < n_alleles:
            a = ancestor.copy()
            for at in rng.integers(0, length, int(rng.integers(1, max_mutations + 1))).tolist():
                a[at] = letters[(int(np.flatnonzero(letters == a[at])[0]) + int(rng.integers(1, 4))) % 4]
            raw = a.tobytes()
            if raw not in seen:
                seen.add(raw)
                records.append((len(records) + 1, raw))
        alleles[locus] = records
    profiles = {}
    for st in range(1, 51):
        profiles.setdefault(tuple(int(x) for x in rng.integers(1, n_alleles + 1, n_loci)), str(st))
    return mlst.Scheme('synth', loci, alleles, profiles)


def write_mlst_scheme(scheme, scheme_dir):
    """The scheme as the files pangenomix_amd.mlst.load_scheme reads"""
    os.makedirs(scheme_dir, exist_ok=True)
    for locus in scheme.loci:
        with open(os.path.join(scheme_dir, locus + '.tfa'), 'wb') as f:
            for number, seq in scheme.alleles[locus]:
                f.write(b'>%s_%d\n%s\n' % (locus.encode('ascii'), number, seq))
    with open(os.path.join(scheme_dir, scheme.name + '.txt'), 'w') as f:
        f.write('\t'.join(['ST'] + list(scheme.loci) + ['clonal_complex']) + '\n')
        for key, st in scheme.profiles.items():
            f.write('\t'.join([st] + [str(n) for n in key] + ['']) + '\n')


def mlst_genome(scheme, path, carried, n_bp=200000, n_contigs=5, seed=0, novel=()):
    """Writes an FNA of n_contigs random contigs, n_bp bases in all, that carries the alleles `carried`: {locus: (number,
    strand)} with strand '+' or '-' (a locus that is no key is absent). A locus in `novel` carries its allele with one base
    changed to a sequence the scheme does not hold. No allele lies across a contig joint. Returns the path."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)
    contigs = [bytearray(letters[rng.integers(0, 4, n_bp // n_contigs)].tobytes()) for _ in range(n_contigs)]
    for i, (locus, (number, strand)) in enumerate(sorted(carried.items())):
        known = {seq for _, seq in scheme.alleles[locus]}
        seq = dict(scheme.alleles[locus])[number]
        at = len(seq) // 2
        while locus in novel and seq in known:
            seq = seq[:at] + b'ACGT'[(b'ACGT'.index(seq[at:at + 1]) + 1) % 4:][:1] + seq[at + 1:]
            at += 1
        contig = contigs[i % n_contigs]
        place = (i // n_contigs + 1) * (len(seq) + 100)
        contig[place:place + len(seq)] = seq if strand == '+' else _revcomp(seq)
    with open(path, 'wb') as f:
        for c, contig in enumerate(contigs):
            f.write(b'>contig%d\n' % (c + 1))
            for j in range(0, len(contig), 80):
                f.write(bytes(contig[j:j + 80]) + b'\n')
    return path


def related_protein_set(seqs, seed=0, substituted=0.1, absent=0.15, indel=0.5, max_indel=8, max_flank=25, prefix='b'):
    """A second protein set derived from `seqs` (bytes each), for pangenomix_amd.ncbi.bidirectional_blast: protein k is left
    out with probability `absent`; a kept one has `substituted` of its sites replaced, with probability `indel` one planted
    deletion or insertion of 1..max_indel residues away from its ends, and unrelated flanks of 0..max_flank random residues
    on either side. Returns (names, sequences, origin): the names are <prefix><position>, origin[i] is the k it came from,
    and the order is shuffled."""
    rng = np.random.default_rng(seed)
    out = []
    for k, raw in enumerate(seqs):
        if rng.random() < absent:
            continue
        s = np.frombuffer(raw, dtype=np.uint8).copy()
        if s.size:
            ProteinSet._mutate(rng, s, substituted)
        if s.size > 2 * max_indel + 4 and rng.random() < indel:
            n = int(rng.integers(1, max_indel + 1))
            at = int(rng.integers(max_indel, s.size - max_indel - n))
            if rng.random() < 0.5:
                s = np.concatenate([s[:at], s[at + n:]])
            else:
                s = np.concatenate([s[:at], AA20[rng.integers(0, 20, n)], s[at:]])
        left, right = (AA20[rng.integers(0, 20, int(rng.integers(0, max_flank + 1)))] for _ in range(2))
        out.append((k, np.concatenate([left, s, right]).tobytes()))
    order = rng.permutation(len(out))
    return (['%s%d' % (prefix, i) for i in range(len(out))], [out[j][1] for j in order],
            np.array([out[j][0] for j in order], dtype=np.int64))


def write_protein_fasta(path, names, seqs, wrap=60):
    with open(path, 'w') as f:
        for name, s in zip(names, seqs):
            s = s.decode('ascii')
            f.write('>%s synthetic protein\n' % name)
            f.write('\n'.join(s[i:i + wrap] for i in range(0, len(s), wrap)) + '\n')
    return path
