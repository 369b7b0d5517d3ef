"""AMR annotation tables (reference amr.py): the CARD ontology as a graph, the resistome of a set of RGI hits, and the
probable hits an annotations file suggests. The reference's names, positional order and defaults; `ctx=None` is the
reference's loop restated -- with its quirks, without one graph search per (hit, drug) -- and a _native.Context gives the
device path:

    build_resistome                            one pgx_graph_reach over the distinct hit AROs and the drugs' AROs
    generate_probable_hits_from_annotations    one pgx_graph_reach for the drug-class terms, one dictionary query for the
                                               exact and the excluded annotations, one pgx_term_scan for every search term

The device path takes regular input only and leaves anything else to the host code unchanged; AMR_PATH_COUNTS says which
path ran. networkx is used where it is importable (construct_aro_to_drug_network then returns an nx.DiGraph, as the
reference does) and needed nowhere: every function that takes G_aro accepts an nx.DiGraph or an AroGraph.
run_rgi, a wrapper of an external program, is not restated."""
from __future__ import print_function
import collections

import numpy as np
import pandas as pd

from . import pangenome as _pg
from .pangenome import generate_annotations, breakdown_feature_name

try:                                                     # optional: nothing here needs it
    import networkx as _nx
except ImportError:                                      # pragma: no cover
    _nx = None

# The drug classes and superclasses of the CARD ontology whose names serve as search terms (facts of the ontology):
# beta-lactam, penam, monobactam, cephalosporin, carbapenem, aminoglycoside, fluoroquinolone, lincosamide, macrolide,
# phenicol, nitrofuran, tetracycline, glycylcycline, diaminopyrimidine, sulfonamide, glycopeptide
DRUG_CLASS_AROS = (
    'ARO:3000007', 'ARO:3000008', 'ARO:0000004', 'ARO:0000032', 'ARO:0000020', 'ARO:0000016', 'ARO:0000001', 'ARO:0000017',
    'ARO:0000000', 'ARO:3000387', 'ARO:3004116', 'ARO:3000050', 'ARO:0000042', 'ARO:3000171', 'ARO:3000282', 'ARO:3000081',
)
_ANTIBIOTIC_ROOT, _ONTOLOGY_ROOT = 'ARO:1000003', 'ARO:1000001'
_FORWARD_RELATIONSHIPS = ('part_of', 'regulates', 'confers_resistance_to_antibiotic', 'confers_resistance_to_drug_class')

# resistome_device / resistome_host, class_terms_device / class_terms_host, screen_device / screen_host: per call
AMR_PATH_COUNTS = collections.Counter()
USE_NETWORKX = None                                      # None: where importable; False: always an AroGraph


class AroGraphError(Exception):
    """what networkx.NetworkXError is where networkx is importable"""


class AroNodeNotFound(AroGraphError):
    """what networkx.NodeNotFound is where networkx is importable"""


NodeNotFound = _nx.NodeNotFound if _nx is not None else AroNodeNotFound
_GraphError = _nx.NetworkXError if _nx is not None else AroGraphError


class AroGraph(object):
    """A directed graph with the few methods this module needs, in the insertion order an nx.DiGraph keeps: `nodes` and
    `edges` (lists), successors(), G[node], add_node(), add_edge(), remove_node(), `in` and len()."""

    def __init__(self):
        self._succ, self._pred = {}, {}

    def add_node(self, node):
        if node not in self._succ:
            self._succ[node], self._pred[node] = {}, {}

    def add_edge(self, u, v):
        self.add_node(u)
        self.add_node(v)
        self._succ[u][v] = None
        self._pred[v][u] = None

    def remove_node(self, node):
        if node not in self._succ:
            raise AroGraphError('The node %s is not in the digraph.' % (node,))
        for v in self._succ.pop(node):
            if v != node:
                del self._pred[v][node]
        for u in self._pred.pop(node):
            if u != node:
                del self._succ[u][node]

    def successors(self, node):
        if node not in self._succ:
            raise AroGraphError('The node %s is not in the digraph.' % (node,))
        return iter(self._succ[node])

    @property
    def nodes(self):
        return list(self._succ)

    @property
    def edges(self):
        return [(u, v) for u, targets in self._succ.items() for v in targets]

    def __contains__(self, node):
        try:
            return node in self._succ
        except TypeError:
            return False

    def __len__(self):
        return len(self._succ)

    def __getitem__(self, node):
        """the successors of `node`, a mapping in insertion order as G[node] of an nx.DiGraph is (KeyError for no node)"""
        return self._succ[node]

    def __iter__(self):
        return iter(self._succ)


def _new_graph():
    if _nx is not None and USE_NETWORKX is not False:
        return _nx.DiGraph()
    return AroGraph()


class _HostPaths(object):
    """Shortest-path node counts by one breadth-first search per distinct source, kept; missing nodes are reported the way
    nx.has_path and nx.shortest_path report them: the source first, then the target."""

    def __init__(self, G):
        self.G, self.from_source = G, {}

    def nodes_on_path(self, source, target):
        G = self.G
        if source not in G:
            raise NodeNotFound('Source %s is not in G' % (source,))
        if target not in G:
            raise NodeNotFound('Target %s is not in G' % (target,))
        dist = self.from_source.get(source)
        if dist is None:
            dist, frontier = {source: 1}, [source]
            while frontier:
                reached = []
                for v in frontier:
                    d = dist[v] + 1
                    for w in G.successors(v):
                        if w not in dist:
                            dist[w] = d
                            reached.append(w)
                frontier = reached
            self.from_source[source] = dist
        return dist.get(target, 0)


class _TablePaths(object):
    """the same answers from the table one pgx_graph_reach call returned; every node asked for is a node"""

    def __init__(self, lengths, row_of, col_of):
        self.lengths, self.row_of, self.col_of = lengths, row_of, col_of

    def nodes_on_path(self, source, target):
        return int(self.lengths[self.row_of[source], self.col_of[target]])


def _graph_csr(G):
    """(index of node, succ_off uint32, succ uint32) of an nx.DiGraph or an AroGraph"""
    nodes = list(G.nodes)
    index = {node: i for i, node in enumerate(nodes)}
    succ, off = [], np.zeros(len(nodes) + 1, dtype=np.uint32)
    for i, node in enumerate(nodes):
        succ.extend(index[w] for w in G.successors(node))
        off[i + 1] = len(succ)
    return index, off, np.array(succ, dtype=np.uint32)


def _device_paths(ctx, G, sources, targets):
    """_TablePaths for the distinct `sources` and `targets`, or None where one of them is not a node (the host code then
    raises at the point of the loop where the reference does)"""
    try:
        sources, targets = list(dict.fromkeys(sources)), list(dict.fromkeys(targets))
        if not all(s in G for s in sources) or not all(t in G for t in targets):
            return None
    except TypeError:
        return None
    index, off, succ = _graph_csr(G)
    lengths = ctx.graph_reach(off, succ, [index[t] for t in targets], [index[s] for s in sources])
    return _TablePaths(lengths, {s: i for i, s in enumerate(sources)}, {t: i for i, t in enumerate(targets)})


def construct_aro_to_drug_network(obo_path):
    """(G_full, aro_names) of a CARD aro.obo (reference :352-425): G_full has a path from an AMR gene's ARO to the ARO of
    every drug and drug class it contributes resistance to, aro_names maps ARO:####### to names. Edges U -> V: U is_a V
    for genes and V is_a U for the descendants of ARO:1000003 (drugs), U part_of / regulates /
    confers_resistance_to_antibiotic / confers_resistance_to_drug_class V, and V has_part U; ARO:1000001 is removed. Both
    passes stop at the first [Typedef] line; an is_a target that is never declared still becomes a node.
    Returns an nx.DiGraph where networkx is importable and an AroGraph (same nodes and edges, same order) otherwise."""
    G_isa, aro_names = _new_graph(), {}
    with open(obo_path, 'r') as f:
        for line in f:
            if line[:8] == 'id: ARO:':
                last_aro = line.strip().split()[1]
                G_isa.add_node(last_aro)
            elif line[:5] == 'name:':
                aro_names[last_aro] = line[6:].strip()
            elif line[:5] == 'is_a:':
                G_isa.add_edge(line.strip().split()[1], last_aro)
            elif line.strip() == '[Typedef]':
                break
    if _ANTIBIOTIC_ROOT not in G_isa:
        raise _GraphError('The node %s is not in the graph.' % _ANTIBIOTIC_ROOT)
    drug_aros, frontier = {_ANTIBIOTIC_ROOT}, [_ANTIBIOTIC_ROOT]
    while frontier:                                      # ARO:1000003 and its descendants
        reached = []
        for v in frontier:
            for w in G_isa.successors(v):
                if w not in drug_aros:
                    drug_aros.add(w)
                    reached.append(w)
        frontier = reached

    G_full = _new_graph()
    with open(obo_path, 'r') as f:
        for line in f:
            if line[:8] == 'id: ARO:':
                last_aro = line.strip().split()[1]
                G_full.add_node(last_aro)
            elif line[:5] == 'is_a:':
                target_aro = line.strip().split()[1]
                if last_aro in drug_aros:                # drug superclass -> drug
                    G_full.add_edge(target_aro, last_aro)
                else:                                    # gene -> gene superclass
                    G_full.add_edge(last_aro, target_aro)
            elif line[:13] == 'relationship:':
                data = line.split()
                relationship_type, target_aro = data[1].strip(), data[2]
                if relationship_type in _FORWARD_RELATIONSHIPS:
                    G_full.add_edge(last_aro, target_aro)
                elif relationship_type == 'has_part':
                    G_full.add_edge(target_aro, last_aro)
            elif line.strip() == '[Typedef]':
                break
    G_full.remove_node(_ONTOLOGY_ROOT)
    return G_full, aro_names


def build_resistome(rgi_txt, drugs, G_aro, skip_loose=True, return_path_lengths=False, ctx=None):
    """(df_rgi, df_aro) of the text file RGI wrote for a non-redundant CDS pan-genome (reference :289-349). df_rgi: the raw
    table, without its Loose hits if skip_loose. df_aro: indexed by allele (ORF_ID), the column ARO and one column per drug
    of `drugs` ({drug: its ARO}), sorted: 1 -- or with return_path_lengths the number of nodes on a shortest path --
    where G_aro has a path from the hit's ARO to the drug's, NaN elsewhere. An allele hit twice prints 'Duplicate hit:' and
    keeps its later ARO in its first place. A hit ARO or a drug ARO that is not a node raises NodeNotFound.
    ctx: a _native.Context for the device path (one pgx_graph_reach for all pairs)."""
    df_rgi = pd.read_csv(rgi_txt, sep='\t')
    if skip_loose:
        df_rgi = df_rgi[df_rgi.Cut_Off != 'Loose']
    df = df_rgi.loc[:, ['ORF_ID', 'ARO']]
    paths = None
    if ctx is not None and len(df) and len(drugs):
        paths = _device_paths(ctx, G_aro, ['ARO:' + str(aro) for aro in df['ARO'].tolist()], list(drugs.values()))
    AMR_PATH_COUNTS['resistome_host' if paths is None else 'resistome_device'] += 1
    if paths is None:
        paths = _HostPaths(G_aro)

    allele_to_drug = {}
    for row in df.itertuples(name=None):
        i, allele, aro = row
        if allele in allele_to_drug:                     # allele mapped to multiple AROs
            print('Duplicate hit:', allele)
        allele_to_drug[allele] = {'ARO': aro}
        for drug, drug_aro in drugs.items():
            path_length = paths.nodes_on_path('ARO:' + str(aro), drug_aro)
            if path_length:
                allele_to_drug[allele][drug] = path_length if return_path_lengths else 1
    column_order = ['ARO'] + sorted(drugs.keys())
    df_aro = pd.DataFrame.from_dict(allele_to_drug, orient='index')
    df_aro = df_aro.reindex(columns=column_order)
    return df_rgi, df_aro


def add_probable_hits(df_aro, df_prob, organism, print_additions=False):
    """df_aro (build_resistome) with the rows of df_prob (generate_probable_hits_from_annotations, after manual curation)
    whose `org` is `organism` and whose drug is a column of df_aro appended in df_aro's format (reference :32-82): the ARO
    column holds '*' + the related AROs for a hit matched to CARD hits (a number, or several joined by ';') and 'Inferred'
    for one inferred from the annotation. The reference's body needs Python 2 (`unicode`) and pandas < 2
    (`DataFrame.append`); this one uses str.isnumeric and pd.concat."""
    drugs_of_interest = df_aro.columns[1:]
    dfp = df_prob[df_prob.org == organism]
    dfp = dfp[dfp.drug.map(lambda x: x in drugs_of_interest)]
    col_order = df_prob.columns.tolist()
    aro_pos = col_order.index('related_aros')
    drug_pos = col_order.index('drug')
    annot_pos = col_order.index('shared_annot')

    df_aro_ext = df_aro.copy(deep=True)
    for row in dfp.itertuples(name=None):
        feature, drug = row[1], row[drug_pos + 1]
        related_aros, annot = str(row[aro_pos + 1]), row[annot_pos + 1]
        if (';' in related_aros) or related_aros.isnumeric():
            aro_label = '*' + related_aros
        else:
            aro_label = 'Inferred'
        if print_additions:
            print(feature, drug, annot)
        df_new = pd.DataFrame.from_dict({feature: {'ARO': aro_label, drug: 1.0}}, orient='index')
        df_aro_ext = pd.concat([df_aro_ext, df_new.reindex(df_aro.columns, axis=1)])
    return df_aro_ext


def _annot_to_amr(df_aro, annotations_file, ctx):
    """(drugs_of_interest, {annotation: {drug: (card-hit alleles joined, their unique AROs joined)}}) (:130-159)"""
    df_aro_annot = generate_annotations(features=df_aro.index, annotation_files=[annotations_file], ctx=ctx)
    df_aro_all = df_aro.copy()
    df_aro_all['annot'] = df_aro_annot.values
    drugs_of_interest = df_aro_all.columns[1:-1]
    annot_to_amr = {}
    for data in df_aro_all.itertuples(name=None):
        card_feature, aro, annot = data[0], data[1], data[-1]
        drug_binary = data[2:-1]                         # 1s or NaNs for drug relevance
        drug_indices = np.argwhere(~np.isnan(drug_binary)).T[0]
        drugs = drugs_of_interest[drug_indices]
        if len(drugs) > 0:
            if annot not in annot_to_amr:
                annot_to_amr[annot] = {drug: [[], []] for drug in drugs}
            for drug in drugs:
                if drug not in annot_to_amr[annot]:
                    annot_to_amr[annot][drug] = [[], []]
                annot_to_amr[annot][drug][0].append(card_feature)
                annot_to_amr[annot][drug][1].append(str(aro))
    for annot in annot_to_amr:
        for drug in annot_to_amr[annot]:
            alleles = ';'.join(annot_to_amr[annot][drug][0])
            unique_aros = ';'.join(set(annot_to_amr[annot][drug][1]))
            annot_to_amr[annot][drug] = (alleles, unique_aros)
    return drugs_of_interest, annot_to_amr


def _class_term_pairs(drugs_of_interest, term_to_aro):
    """the (drug class, drug) pairs the loop of _search_terms asks about, for one pgx_graph_reach"""
    targets = []
    for drug in drugs_of_interest:
        for subdrug in [drug] + (drug.split('/') if '/' in drug else []):
            if subdrug in term_to_aro:
                targets.append(term_to_aro[subdrug])
    return list(DRUG_CLASS_AROS), targets


def _search_terms(drugs_of_interest, check_drug_mentions, G_aro, aro_names, drug_to_aro, manual_annots, paths):
    """{drug: set of terms} (:161-199): the drug, the parts of a combination, the names of its drug classes, the names
    drug_to_aro gives, and manual_annots"""
    term_to_aro = {v: k for k, v in aro_names.items()}
    search_terms = {}
    if check_drug_mentions:
        for drug in drugs_of_interest:
            search_terms[drug] = [drug]
            if '/' in drug:                              # combination therapy, check for individual drugs
                search_terms[drug] += drug.split('/')
            if G_aro is not None:
                class_terms = []
                for drug_class_aro in DRUG_CLASS_AROS:
                    for subdrug in search_terms[drug]:
                        if subdrug in term_to_aro:
                            drug_aro = term_to_aro[subdrug]
                            if paths.nodes_on_path(drug_class_aro, drug_aro):
                                drug_class = aro_names[drug_class_aro]
                                drug_class = drug_class.replace('antibiotic', '').strip()
                                class_terms.append(drug_class)
                search_terms[drug] += class_terms
    for drug, aro in drug_to_aro.items():
        if drug in drugs_of_interest:
            if drug not in search_terms:
                search_terms[drug] = []
            search_terms[drug].append(aro_names[aro])
    curated_terms = [x for x in manual_annots.keys() if x in drugs_of_interest]
    for drug in curated_terms:
        if drug not in search_terms:
            search_terms[drug] = manual_annots[drug]
        else:
            search_terms[drug] += list(manual_annots[drug])
    return {k: set(v) for k, v in search_terms.items()}


def _screen_host(annotations_file, excluded_annots, annot_to_amr, drugs_of_interest, search_terms):
    """the rows of df_prob in line, annotation, exact-match-drug and drug-of-interest order (:202-225)"""
    selected_features = []
    with open(annotations_file) as f:
        for line in f:
            data = line.strip().split('\t')
            feature, annots = data[0], data[1:]
            annots = [x for x in annots if (x not in excluded_annots)]
            for annot in annots:
                annot_lower = annot.lower()
                if annot in annot_to_amr:                # identical annotation to a CARD hit's
                    for drug in annot_to_amr[annot]:
                        card_hits, related_aros = annot_to_amr[annot][drug]
                        selected_features.append((feature, drug, annot, card_hits, related_aros))
                for drug in drugs_of_interest:           # terms from the ontology and from curation
                    if drug in search_terms:
                        for search_term in search_terms[drug]:
                            if search_term in annot or search_term.lower() in annot_lower:
                                selected_features.append((feature, drug, annot, np.nan, search_term))
                                break
    return selected_features


def _is_ascii_str(x):
    return isinstance(x, str) and x.isascii()


def _screen_device(ctx, annotations_file, excluded_annots, annot_to_amr, drugs_of_interest, search_terms):
    """The same rows, or None for input the device path does not take: the exact and the excluded annotations are one
    dictionary query and every term of every drug one pgx_term_scan over the annotation fields of the file's bytes, after
    which only the fields with a dictionary hit or a non-zero mask are visited."""
    from . import _native
    with open(annotations_file, 'rb') as f:
        data = f.read()
    if not _pg._plain_ascii(data) or len(data) >= (1 << 32):
        return None                                      # non-ASCII bytes, '\r', what only str.strip() takes off
    arr = np.frombuffer(data, dtype=np.uint8)
    ls, le = _pg._line_spans(arr)
    space = _pg._PROX_SPACE
    if ls.size and ((le <= ls).any() or space[arr[ls]].any() or space[arr[np.maximum(le, 1) - 1]].any()):
        return None                                      # strip() would change a line
    # the terms, folded, each once: a term that is not ASCII text, or more of them than the kernel holds, goes to the host
    per_drug, term_id, term_bytes = [], {}, []
    for drug in drugs_of_interest:
        if drug in search_terms:
            ids = []
            for term in search_terms[drug]:              # (the set's own order decides which term is reported)
                if not _is_ascii_str(term):
                    return None
                key = term.lower().encode('ascii')
                if key not in term_id:
                    term_id[key] = len(term_bytes)
                    term_bytes.append(key)
                ids.append((term, term_id[key]))
            per_drug.append((drug, ids))
    if len(term_bytes) > _native.TERM_MAX_TERMS or sum(map(len, term_bytes)) > _native.TERM_MAX_BYTES:
        return None
    # the annotation fields: what follows each tab, up to the next tab or the end of the line
    tabs = np.flatnonzero(arr == 9)
    if tabs.size >= (1 << 24):
        return None
    breaks = np.sort(np.concatenate((tabs, le)))
    f_start = tabs + 1
    f_end = breaks[np.searchsorted(breaks, tabs, side='right')] if tabs.size else tabs
    f_line = np.searchsorted(ls, tabs, side='right') - 1
    # a key that is no ASCII string equals no field of an ASCII file
    keys = list(dict.fromkeys([a for a in annot_to_amr if _is_ascii_str(a)] + [x for x in excluded_annots if _is_ascii_str(x)]))
    hit = np.full(tabs.size, -1, dtype=np.int32)
    if keys and tabs.size:
        k_blob, k_off = _pg._blob([k.encode('ascii') for k in keys])
        ctx.dict_load(k_blob, k_off, want_first=False)
        hit = ctx.dict_query(*_pg._spans_blob(arr, f_start, f_end))
    if term_bytes and tabs.size:
        t_blob, t_off = _pg._blob(term_bytes)
        mask = ctx.term_scan(arr, f_start.astype(np.uint64), (f_end - f_start).astype(np.uint32), t_blob,
                             t_off.astype(np.uint32), _native.TERM_FOLD_ASCII)
    else:
        mask = np.zeros((tabs.size, 0), dtype=np.uint64)
    selected_features = []
    for j in np.flatnonzero((hit >= 0) | mask.any(axis=1)).tolist():
        annot = data[int(f_start[j]):int(f_end[j])].decode('ascii')
        if annot in excluded_annots:
            continue
        line = int(f_line[j])
        feature = data[int(ls[line]):int(le[line])].split(b'\t', 1)[0].decode('ascii')
        if annot in annot_to_amr:
            for drug in annot_to_amr[annot]:
                card_hits, related_aros = annot_to_amr[annot][drug]
                selected_features.append((feature, drug, annot, card_hits, related_aros))
        words = mask[j].tolist()
        for drug, ids in per_drug:
            for term, t in ids:
                if (words[t >> 6] >> (t & 63)) & 1:
                    selected_features.append((feature, drug, annot, np.nan, term))
                    break
    return selected_features


def generate_probable_hits_from_annotations(df_aro, annotations_file, exclude=['hypothetical protein'],
                                            check_drug_mentions=True, G_aro=None, aro_names={}, drug_to_aro={},
                                            manual_annots={}, ignore_case=True, ctx=None):
    """df_prob: the features of an annotations file (pangenome.extract_annotations) that probably relate to AMR, because
    an annotation of theirs equals that of a CARD hit of df_aro (build_resistome) or mentions a drug, a part of a
    combination, one of the drug's classes (G_aro and aro_names from construct_aro_to_drug_network; the sixteen
    DRUG_CLASS_AROS, 'antibiotic' taken out of their names), a name drug_to_aro gives or a phrase of manual_annots
    ({drug: phrases}) (reference :85-244). Annotations in `exclude` are ignored. Columns: feature, drug, shared_annot,
    card_hits, related_aros, shared_gene; one row per (annotation, drug) for the first matching term in the order the
    drug's set of terms iterates, rows in line, annotation, exact-match-drug and drug-of-interest order, then sorted by
    drug. The dictionary of search terms is printed.
    ignore_case: kept for the signature and without effect, as in the reference, whose `found` is never used: a term
    matches iff `term in annot or term.lower() in annot.lower()`, which for ASCII text is `term.lower() in annot.lower()`.
    ctx: a _native.Context for the device path. Files with non-ASCII bytes, '\\r', or a line strip() would change other
    than by its newline, terms that are not ASCII text and more terms than pgx_term_scan holds go to the host loop."""
    drugs_of_interest, annot_to_amr = _annot_to_amr(df_aro, annotations_file, ctx)
    excluded_annots = set(exclude)

    paths = None
    if check_drug_mentions and G_aro is not None:
        if ctx is not None:
            try:
                sources, targets = _class_term_pairs(drugs_of_interest, {v: k for k, v in aro_names.items()})
                paths = _device_paths(ctx, G_aro, sources, targets) if targets else None
            except (TypeError, AttributeError):          # a drug that is no string: the host loop raises what it raises
                paths = None
        AMR_PATH_COUNTS['class_terms_host' if paths is None else 'class_terms_device'] += 1
        if paths is None:
            paths = _HostPaths(G_aro)
    search_terms = _search_terms(drugs_of_interest, check_drug_mentions, G_aro, aro_names, drug_to_aro, manual_annots, paths)
    print(search_terms)

    selected_features = None
    if ctx is not None:
        selected_features = _screen_device(ctx, annotations_file, excluded_annots, annot_to_amr, drugs_of_interest, search_terms)
    AMR_PATH_COUNTS['screen_host' if selected_features is None else 'screen_device'] += 1
    if selected_features is None:
        selected_features = _screen_host(annotations_file, excluded_annots, annot_to_amr, drugs_of_interest, search_terms)
    columns = ('feature', 'drug', 'shared_annot', 'card_hits', 'related_aros')
    df_prob = pd.DataFrame(columns=columns, data=selected_features)

    shared_gene = []
    for row in df_prob.itertuples(name=None):
        probable_feature, related_hits = row[1], row[4]
        name, ctype, cnum, vtype, vnum = breakdown_feature_name(probable_feature)
        probable_cluster = name + '_' + ctype + str(cnum)
        is_shared = False
        if pd.notnull(related_hits):                     # hit from similarity to CARD hit
            for hit in related_hits.split(';'):
                name, ctype, cnum, vtype, vnum = breakdown_feature_name(hit)
                related_cluster = name + '_' + ctype + str(cnum)
                if related_cluster == probable_cluster:
                    is_shared = True
                    break
        shared_gene.append(is_shared)
    df_prob['shared_gene'] = shared_gene
    df_prob.sort_values(by='drug', inplace=True)
    return df_prob
