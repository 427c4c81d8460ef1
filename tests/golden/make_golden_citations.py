"""Generate tests/golden/gpr_definitions.json FROM THE REFERENCE ITSELF: the line count of the reference's ``gpras/gpr.py`` and
the line span (first, last) of every function and class it defines, which tests/test_citations.py checks the ``gpr.py:A-B``
citations of the boundary documents against.  Names and line numbers only; no source text is recorded.

    python tests/golden/make_golden_citations.py <checkout of fema-ffrd/gpras>
"""

import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main(reference):
    with open(os.path.join(reference, "gpras", "gpr.py")) as f:
        src = f.read()
    spans = {}
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            spans.setdefault(node.name, []).append([node.lineno, node.end_lineno])
    n_lines = src.count("\n") + 1
    rows = ",\n".join(f"  {json.dumps(k)}: {json.dumps(sorted(v))}" for k, v in sorted(spans.items()))
    path = os.path.join(HERE, "gpr_definitions.json")
    with open(path, "w") as f:
        f.write(f'{{\n "file": "gpras/gpr.py",\n "n_lines": {n_lines},\n "definitions": {{\n{rows}\n }}\n}}\n')
    print(f"wrote {path}: {len(spans)} names, {n_lines} lines")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
