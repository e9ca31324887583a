// Maintained by hand (tools/gen_rust_shim.py generates only src/lib.rs of this crate)
// HALO2_MI355X_LIB_DIR = <this repository>/halo2-experiments_amd/csrc (where `make` leaves libhalo2_mi355x.so)
fn main() {
    let dir = std::env::var("HALO2_MI355X_LIB_DIR")
        .expect("set HALO2_MI355X_LIB_DIR to <repo>/halo2-experiments_amd/csrc (the directory of libhalo2_mi355x.so)");
    println!("cargo:rustc-link-search=native={dir}");
    println!("cargo:rustc-link-lib=dylib=halo2_mi355x");
    println!("cargo:rustc-link-arg=-Wl,-rpath,{dir}");
    println!("cargo:rerun-if-env-changed=HALO2_MI355X_LIB_DIR");
}
