"""Writes tests/golden/amr: what the reference's construct_aro_to_drug_network, build_resistome and
generate_probable_hits_from_annotations (amr.py:85-425) returned and printed on a hand-written ontology of a few dozen terms,
an RGI table and an annotations file. Needs the reference checkout -- its directory is the first argument or
$PANGENOMIX_REFERENCE; nothing of it is copied -- and networkx, which the reference imports. The reference's amr.py does
`from pangenome import ...`, so its package directory goes on sys.path as well.

The inputs hold: the sixteen drug-class ids and ARO:1000001 / ARO:1000003 (the reference raises without them), a combination
drug with has_part, an is_a target that is never declared, a relationship type that is ignored, a gene with two routes of
different length to one drug, and terms after [Typedef]; an RGI table with a Loose row, an ORF_ID hit twice and a hit that
relates to no drug; an annotations file with a line of two annotations, an excluded annotation, an allele whose annotation
comes from its cluster's line, and a term that matches only when case is ignored.
Recorded: nodes, edges and aro_names in the reference's order, df_aro in both flavours, what build_resistome printed, the
search terms (as sorted lists: the printed sets have no order of their own) and df_prob with its index. The fixture is built
so that no (annotation, drug) has two unique AROs or matches two different terms: then nothing recorded depends on the order
in which a set of strings iterates, which changes from process to process."""
import contextlib
import io
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ['PANGENOMIX_REFERENCE']
sys.path.insert(0, REFERENCE)
sys.path.insert(0, os.path.join(REFERENCE, 'pangenomix'))
for _name in ('statsmodels', 'statsmodels.stats', 'Bio', 'Bio.SeqIO'):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules['statsmodels'].stats = sys.modules['statsmodels.stats']
sys.modules['Bio'].SeqIO = sys.modules['Bio.SeqIO']

import pangenomix.amr as ref_amr                          # noqa: E402

OUT = os.path.join(HERE, 'amr')

CLASSES = [('ARO:3000007', 'beta-lactam antibiotic', None), ('ARO:3000008', 'penam', 'ARO:3000007'),
           ('ARO:0000004', 'monobactam', 'ARO:3000007'), ('ARO:0000032', 'cephalosporin', 'ARO:3000007'),
           ('ARO:0000020', 'carbapenem', 'ARO:3000007'), ('ARO:0000016', 'aminoglycoside antibiotic', None),
           ('ARO:0000001', 'fluoroquinolone antibiotic', None), ('ARO:0000017', 'lincosamide antibiotic', None),
           ('ARO:0000000', 'macrolide antibiotic', None), ('ARO:3000387', 'phenicol antibiotic', None),
           ('ARO:3004116', 'nitrofuran antibiotic', None), ('ARO:3000050', 'tetracycline antibiotic', None),
           ('ARO:0000042', 'glycylcycline', 'ARO:3000050'), ('ARO:3000171', 'diaminopyrimidine antibiotic', None),
           ('ARO:3000282', 'sulfonamide antibiotic', None), ('ARO:3000081', 'glycopeptide antibiotic', None)]
DRUG_TERMS = [('ARO:3000637', 'ampicillin', 'ARO:3000008'), ('ARO:0000062', 'ceftriaxone', 'ARO:0000032'),
              ('ARO:0000014', 'gentamicin', 'ARO:0000016'), ('ARO:0000036', 'ciprofloxacin', 'ARO:0000001'),
              ('ARO:3000188', 'trimethoprim', 'ARO:3000171'), ('ARO:3000324', 'sulfamethoxazole', 'ARO:3000282'),
              ('ARO:0000051', 'tetracycline', 'ARO:3000050'), ('ARO:0000028', 'vancomycin', 'ARO:3000081')]


def term(aro, name, is_a=(), relationships=(), extra=()):
    lines = ['[Term]', 'id: ' + aro, 'name: ' + name]
    lines += ['is_a: %s ! parent' % x for x in is_a]
    lines += ['relationship: %s %s ! target' % r for r in relationships]
    return '\n'.join(lines + list(extra)) + '\n\n'


def obo():
    text = 'format-version: 1.2\nontology: aro\n\n'
    text += term('ARO:1000001', 'process or component of antibiotic biology or chemistry')
    text += term('ARO:1000003', 'antibiotic molecule', ['ARO:1000001'])
    text += term('ARO:3000000', 'determinant of antibiotic resistance', ['ARO:1000001'])
    for aro, name, parent in CLASSES:
        text += term(aro, name, [parent or 'ARO:1000003'])
    for aro, name, parent in DRUG_TERMS:
        text += term(aro, name, [parent])
    text += term('ARO:3000707', 'antibiotic mixture', ['ARO:1000003'])
    text += term('ARO:3004024', 'trimethoprim-sulfamethoxazole', ['ARO:3000707'],
                 [('has_part', 'ARO:3000188'), ('has_part', 'ARO:3000324')])
    text += term('ARO:3000001', 'beta-lactamase', ['ARO:3000000'], [('confers_resistance_to_drug_class', 'ARO:3000007')])
    text += term('ARO:3000014', 'TEM beta-lactamase', ['ARO:3000001'])
    # two routes to ampicillin: the direct edge (2 nodes) and up the families, over to the class, down the drug tree (6)
    text += term('ARO:3000873', 'TEM-1', ['ARO:3000014'], [('confers_resistance_to_antibiotic', 'ARO:3000637')])
    text += term('ARO:3000016', 'CTX-M beta-lactamase', ['ARO:3000001'])
    text += term('ARO:3001878', 'CTX-M-15', ['ARO:3000016'], [('confers_resistance_to_antibiotic', 'ARO:0000062')])
    text += term('ARO:3000322', 'AAC(3)', ['ARO:3000000'], [('confers_resistance_to_drug_class', 'ARO:0000016')])
    text += term('ARO:3002533', 'AAC(3)-IIa', ['ARO:3000322'])
    text += term('ARO:3001218', 'trimethoprim resistant dihydrofolate reductase dfr', ['ARO:3000000'],
                 [('confers_resistance_to_antibiotic', 'ARO:3000188')])
    text += term('ARO:3002860', 'dfrA17', ['ARO:3001218'])
    text += term('ARO:3000384', 'AcrAB-TolC', ['ARO:3000000'],
                 [('confers_resistance_to_drug_class', 'ARO:0000001'), ('confers_resistance_to_drug_class', 'ARO:3000050')])
    text += term('ARO:3000216', 'acrB', ['ARO:3000000'], [('part_of', 'ARO:3000384')])
    text += term('ARO:3000263', 'marA', ['ARO:3000000'], [('regulates', 'ARO:3000384')])
    # an is_a target that is never declared, and a relationship type that is ignored
    text += term('ARO:3003000', 'orphan determinant', ['ARO:9999999'], [('participates_in', 'ARO:3000007')],
                 ['synonym: "odd" EXACT []'])
    text += '[Typedef]\nid: part_of\nname: part_of\n\n'
    text += term('ARO:8888888', 'a term after the type definitions', ['ARO:3000001'], [('part_of', 'ARO:3000384')])
    return text


RGI_COLUMNS = ['ORF_ID', 'Contig', 'Cut_Off', 'Best_Hit_ARO', 'ARO']
RGI_ROWS = [('Eco_C10A0', 'c1', 'Strict', 'TEM-1', 3000873),
            ('Eco_C10A1', 'c1', 'Perfect', 'TEM-1', 3000873),
            ('Eco_C11A0', 'c2', 'Strict', 'CTX-M-15', 3001878),
            ('Eco_C12A0', 'c2', 'Loose', 'AAC(3)-IIa', 3002533),                  # dropped by skip_loose
            ('Eco_C12A1', 'c3', 'Strict', 'AAC(3)-IIa', 3002533),
            ('Eco_C13A0', 'c3', 'Strict', 'dfrA17', 3002860),
            ('Eco_C14A0', 'c4', 'Strict', 'orphan determinant', 3003000),          # relates to no drug
            ('Eco_C10A0', 'c4', 'Strict', 'CTX-M-15', 3001878),                    # hit twice: the later ARO, the first place
            ('Eco_C15A0', 'c5', 'Strict', 'acrB', 3000216),
            ('Eco_C16A2', 'c5', 'Strict', 'marA', 3000263)]
DRUGS = {'ampicillin': 'ARO:3000637', 'ceftriaxone': 'ARO:0000062', 'gentamicin': 'ARO:0000014',
         'ciprofloxacin': 'ARO:0000036', 'trimethoprim/sulfamethoxazole': 'ARO:3004024', 'tetracycline': 'ARO:0000051',
         'vancomycin': 'ARO:0000028'}
ANNOTATIONS = [('Eco_C10A0', ['Class A beta-lactamase (EC 3.5.2.6)']),
               ('Eco_C10A1', ['Class A beta-lactamase (EC 3.5.2.6)', 'TEM family']),          # two annotations
               ('Eco_C11A0', ['Class A beta-lactamase (EC 3.5.2.6)']),
               ('Eco_C12A1', ['AAC(3) family N-acetyltransferase']),
               ('Eco_C13A0', ['Dihydrofolate reductase (EC 1.5.1.3)']),
               ('Eco_C14A0', ['hypothetical protein']),
               ('Eco_C15A0', ['Multidrug efflux pump subunit AcrB']),
               ('Eco_C16', ['Transcriptional activator MarA']),                               # Eco_C16A2 takes this one
               ('Eco_C10A5', ['Class A beta-lactamase (EC 3.5.2.6)']),                        # the cluster of a CARD hit
               ('Eco_C20A0', ['Class A beta-lactamase (EC 3.5.2.6)']),
               ('Eco_C21A0', ['hypothetical protein', 'GENTAMICIN 3-N-acetyltransferase']),   # excluded; case ignored
               ('Eco_C22A0', ['Dihydrofolate reductase (EC 1.5.1.3)', 'Trimethoprim-insensitive enzyme']),
               ('Eco_C23A0', ['Tetracycline efflux MFS transporter Tet(A)']),
               ('Eco_C24A0', ['DNA gyrase subunit A']),                                       # a manual phrase
               ('Eco_C25A0', ['Sulfonamide-resistant dihydropteroate synthase']),             # a class of a combination's part
               ('Eco_C26A0', ['Transcriptional activator MarA', 'Glutamate synthase']),
               ('Eco_C27A0', ['Ribosomal protein L2'])]
PROBABLE_ARGS = {'exclude': ['hypothetical protein'], 'drug_to_aro': {'gentamicin': 'ARO:3000322'},
                 'manual_annots': {'ciprofloxacin': ['gyrase'], 'colistin': ['never a drug of interest']}}


def captured(fn, *args, **kwargs):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        result = fn(*args, **kwargs)
    return result, out.getvalue()


def main():
    os.makedirs(OUT, exist_ok=True)
    paths = {name: os.path.join(OUT, name) for name in ('aro.obo', 'rgi.txt', 'annotations.tsv')}
    with open(paths['aro.obo'], 'w') as f:
        f.write(obo())
    with open(paths['rgi.txt'], 'w') as f:
        f.write('\t'.join(RGI_COLUMNS) + '\n')
        f.writelines('\t'.join(str(x) for x in row) + '\n' for row in RGI_ROWS)
    with open(paths['annotations.tsv'], 'w') as f:
        f.writelines('\t'.join([feature] + annots) + '\n' for feature, annots in ANNOTATIONS)

    G, aro_names = ref_amr.construct_aro_to_drug_network(paths['aro.obo'])
    (df_rgi, df_aro), printed = captured(ref_amr.build_resistome, paths['rgi.txt'], DRUGS, G)
    (_, df_len), printed_len = captured(ref_amr.build_resistome, paths['rgi.txt'], DRUGS, G, return_path_lengths=True)
    assert printed == printed_len == 'Duplicate hit: Eco_C10A0\n'
    assert df_len.loc['Eco_C10A1', 'ampicillin'] == 2 and df_len.loc['Eco_C10A0', 'ampicillin'] == 6
    assert df_aro['vancomycin'].isna().all() and df_aro.loc['Eco_C14A0'].isna().sum() == len(DRUGS)
    df_prob, printed_prob = captured(ref_amr.generate_probable_hits_from_annotations, df_aro, paths['annotations.tsv'],
                                     G_aro=G, aro_names=aro_names, **PROBABLE_ARGS)
    search_terms = eval(printed_prob, {'__builtins__': {}})              # the printed dict of sets
    # nothing recorded may depend on the order a set of strings iterates in
    for aros in df_prob['related_aros'][df_prob['card_hits'].notna()]:
        assert ';' not in aros, aros
    for _, annots in ANNOTATIONS:
        for annot in annots:
            for drug, terms in search_terms.items():
                assert len({t for t in terms if t.lower() in annot.lower()}) <= 1, (annot, drug)
    assert (df_prob['related_aros'] == 'gentamicin').any() and df_prob['shared_gene'].any()

    df_aro.to_csv(os.path.join(OUT, 'df_aro.tsv'), sep='\t')
    df_len.to_csv(os.path.join(OUT, 'df_aro_lengths.tsv'), sep='\t')
    df_prob.to_csv(os.path.join(OUT, 'df_prob.tsv'), sep='\t')
    with open(os.path.join(OUT, 'expected.json'), 'w') as f:
        json.dump({'nodes': list(G.nodes), 'edges': [list(e) for e in G.edges], 'aro_names': aro_names, 'drugs': DRUGS,
                   'probable_args': PROBABLE_ARGS, 'resistome_stdout': printed,
                   'search_terms': {k: sorted(v) for k, v in search_terms.items()}}, f, indent=1)
    print('nodes %d, edges %d, df_aro %r, df_prob %r' % (len(G), G.number_of_edges(), df_aro.shape, df_prob.shape))


if __name__ == '__main__':
    main()
