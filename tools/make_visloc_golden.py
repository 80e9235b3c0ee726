"""Records the `from <module> import <names>` statements of the reference's visloc.py that the engine serves (dust3r.* and
dust3r_visloc.localization / .evaluation) into tests/golden/visloc_imports.json, which tests/test_visloc_cpu.py replays against the
INTEGRATION.md section 1 aliases.

    python tools/make_visloc_golden.py /path/to/reference/checkout"""
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'visloc_imports.json')
SERVED = ('dust3r.', 'dust3r_visloc.localization', 'dust3r_visloc.evaluation')


def main(reference):
    with open(os.path.join(reference, 'visloc.py')) as fh:
        tree = ast.parse(fh.read())
    imports = [[node.module, [a.name for a in node.names]] for node in tree.body
               if isinstance(node, ast.ImportFrom) and node.module and node.module.startswith(SERVED)]
    with open(OUT, 'w') as fh:
        json.dump(dict(source='visloc.py', imports=imports), fh, indent=1)
        fh.write('\n')
    print(OUT, imports)


if __name__ == '__main__':
    main(sys.argv[1])
