!> `refit` with several fields in one call on a grid that takes the nested-dissection factorisation: 3-D, 16^3 nodes, 10^4
!! weighted points of the seeded Park-Miller stream, xtrap = 1 (the shape of parity case "3d16" of tests/cases.py).  After one
!! `initialize`, three fields cos((3 + k)(x1 + x2 + x3)), k = 0, 1, 2, are refitted in ONE call -- the library solves them in
!! sweeps of the factor that the fields share -- and one by one: every field of the call must be the bits of its own
!! single-field refit.  (GPU)
program test_refitbatch
    use splpak_module, wp => splpak_wp
    implicit none
    integer,parameter :: m = 10000, ncol = 4096, nf = 3
    integer :: nodes(3), ierror, i, k, nbad
    real(wp) :: xdata(3,m), ydata(m), wdata(m), xmin(3), xmax(3), u(5), sx
    real(wp),allocatable :: fields(:,:), cmany(:,:), cone(:), coef(:), work(:)
    integer(8) :: s
    type(splpak_type) :: solver

    nbad = 0
    allocate(fields(m,nf), cmany(ncol,nf), cone(ncol), coef(ncol), work(ncol*(ncol+1)))
    s = 42_8
    do i = 1, m
        do k = 1, 5
            call draw(u(k))
        end do
        xdata(:,i) = u(1:3)
        ydata(i) = sin(3.0_wp*u(1) + 1.0_wp) + sin(3.0_wp*u(2) + 2.0_wp) + sin(3.0_wp*u(3) + 3.0_wp) + 0.01_wp*(u(4) - 0.5_wp)
        wdata(i) = 0.5_wp + u(5)
        sx = u(1) + u(2) + u(3)
        do k = 1, nf
            fields(i,k) = cos(real(2 + k, wp)*sx)
        end do
    end do
    xmin = 0.0_wp; xmax = 1.0_wp; nodes = [16,16,16]

    call solver%initialize(3,xdata,3,ydata,wdata,m,xmin,xmax,nodes,1.0_wp,coef,ncol,work,size(work),ierror)
    if (ierror /= 0) error stop 'fit failed'
    cmany = -1.0_wp
    call solver%refit(fields,cmany,ierror,nfields=nf)
    if (ierror /= 0) error stop 'refit of three fields failed'
    do k = 1, nf
        call solver%refit(fields(:,k),cone,ierror)
        if (ierror /= 0) error stop 'single refit failed'
        write(*,'(A,I2,A,ES12.3)') ' field ', k, ': max |many - single| = ', maxval(abs(cmany(:,k) - cone))
        if (any(cmany(:,k) /= cone)) call fail('a field of the call is not the bits of its single-field refit')
        if (.not. (maxval(abs(cone)) > 0.0_wp)) call fail('a field came back zero')
    end do
    call solver%destroy()
    if (nbad /= 0) error stop 'test_refitbatch FAILED'
    write(*,*) 'PASS test_refitbatch'
contains
    subroutine draw(v)
        real(wp),intent(out) :: v
        s = mod(48271_8*s, 2147483647_8)
        v = real(real(s,8)/2147483647.0_8, wp)
    end subroutine draw
    subroutine fail(what)
        character(len=*),intent(in) :: what
        write(*,*) 'FAILED: ', what
        nbad = nbad + 1
    end subroutine fail
end program test_refitbatch
