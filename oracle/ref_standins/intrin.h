// oracle/ref_standins -- TEST INFRASTRUCTURE ONLY.  Stand-in for a platform/SDK header that the reference's template/precomp.h includes
// unconditionally; written for this project, it holds only what that header needs to parse (see oracle/Makefile, _ref/libref_hotpath.so).
// Nothing from this header is used by the code that is compiled.
