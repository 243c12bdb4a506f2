"""Write tests/golden/demo_surface.json: the import surface of the reference's two demos (demo/build_submaps.py,
demo/align_submaps.py) as data, so that tests/test_demo_surface.py runs without the reference checkout.

Per demo it records names only: the module-level import statements (module, imported names, aliases), the names the
script defines at module level, and for each of its functions the names that function loads and does not bind itself
(the free names the package and the imports have to provide).

    python tools/make_demo_surface_golden.py <path of the reference checkout>
"""
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMOS = ("build_submaps.py", "align_submaps.py")


def surface(src):
    tree = ast.parse(src)
    imports = []
    for n in tree.body:
        if isinstance(n, ast.Import):
            imports.append({"import": [[a.name, a.asname] for a in n.names]})
        elif isinstance(n, ast.ImportFrom):
            imports.append({"from": n.module, "level": n.level, "names": [[a.name, a.asname] for a in n.names]})
    defined = {n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    for node in tree.body:
        if isinstance(node, ast.Assign):
            defined |= {t.id for t in node.targets if isinstance(t, ast.Name)}
    functions = {}
    for fn in (n for n in tree.body if isinstance(n, ast.FunctionDef)):
        local = {a.arg for a in fn.args.args + fn.args.kwonlyargs}
        for node in ast.walk(fn):
            if isinstance(node, ast.Name) and isinstance(node.ctx, ast.Store):
                local.add(node.id)
            elif isinstance(node, (ast.For, ast.comprehension)):
                local |= {t.id for t in ast.walk(node.target) if isinstance(t, ast.Name)}
            elif isinstance(node, ast.withitem) and node.optional_vars is not None:
                local |= {t.id for t in ast.walk(node.optional_vars) if isinstance(t, ast.Name)}
        loads = {node.id for node in ast.walk(fn) if isinstance(node, ast.Name) and isinstance(node.ctx, ast.Load)}
        functions[fn.name] = sorted(loads - local)
    return {"imports": imports, "defined": sorted(defined), "functions": functions}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    out = {d: surface(open(os.path.join(ref, "demo", d)).read()) for d in DEMOS}
    path = os.path.join(ROOT, "tests", "golden", "demo_surface.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
