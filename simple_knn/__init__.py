"""`import simple_knn` resolves to the MI355X implementation (materialrefgs_amd.knn -> libmrgs.so).

The reference's CUDA extension is the package `simple_knn` with one compiled module, `simple_knn._C` (submodules/simple-knn/setup.py);
with this repository's root on the path instead, `simple_knn/_C.py` takes that module's place.  See INTEGRATION.md.
"""
